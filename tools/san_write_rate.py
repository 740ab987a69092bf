"""Rate of writing SAN on the device (sc_moves_to_san_device: walk + one wavefront per ply) next to reading it back
(sc_encode_san_device with only moves + status: the parser's latency chain), on the 256-game trace set of
tools/encode_device_rate.py.  Prints one JSON line and appends it to profiles/san_write_rate_<date>.jsonl (--out).

  python tools/san_write_rate.py [--reps 7] [--out FILE]

rows:
  san_write   sc_moves_to_san_device: the moves' upload, ply index, walk (k_replay_raw), k_san_write, k_san_clip, status codes
  san_moves   sc_encode_san_device with only moves + status on the writer's own text of the same games (suffixes stripped, as
              the tokenizer leaves them): the tokens' upload and the parser kernel
  device_ms   HIP events recorded on the caller's stream around the call;  call_ms: host wall time of the call plus the wait
              for its stream.  Medians over --reps regions after one warm-up call, with [min, max]; inputs packed and buffers
              allocated once, outside the timing.
Every game must render (status 0), and the parser must read the writer's text back to the moves it was made of."""
import argparse
import ctypes as C
import datetime
import json
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smart-chess-rust_amd"))

import numpy as np  # noqa: E402

import scamd  # noqa: E402
import scamd.san  # noqa: E402
from encode_device_rate import trace_set  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "san_write_rate_%s.jsonl" % datetime.date.today().isoformat()))
    args = ap.parse_args()
    L = scamd.lib()
    if L.sc_device_count() <= 0:
        raise SystemExit("no HIP device")
    eng = scamd.Engine(args.blocks, args.channels, seed=1)
    games = trace_set(eng)
    eng.close()
    hip = scamd.hip_runtime()
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    stream, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    bufs = []

    def alloc(nbytes):
        q = C.c_void_p()
        assert hip.hipMalloc(C.byref(q), max(int(nbytes), 1)) == 0
        bufs.append(q)
        return q

    def download(q, shape, dtype):
        a = np.zeros(shape, dtype)
        assert hip.hipMemcpy(p(a), q, a.nbytes, 2) == 0
        return a

    mv = np.asarray([scamd.uci_move(s[0]) if isinstance(s[0], str) else int(s[0]) for g in games for s in g], np.uint16)
    off = np.zeros(len(games) + 1, np.uint32)
    off[1:] = np.cumsum([len(g) for g in games])
    n, P = len(games), int(off[-1])
    d_tok, d_moves, st_write, st_parse = alloc(P * 8), alloc(P * 2), alloc(n * 4), alloc(n * 4)

    def timed(call):
        def checked():
            rc = call()
            assert rc == 0, L.sc_last_error().decode()
        checked()
        assert hip.hipStreamSynchronize(stream) == 0
        call_ms, dev_ms = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            hip.hipEventRecord(e0, stream)
            checked()
            hip.hipEventRecord(e1, stream)
            assert hip.hipStreamSynchronize(stream) == 0
            call_ms.append((time.perf_counter() - t0) * 1e3)
            ms = C.c_float(0)
            hip.hipEventElapsedTime(C.byref(ms), e0, e1)
            dev_ms.append(ms.value)
        c, dm = statistics.median(call_ms), statistics.median(dev_ms)
        return {"call_ms": round(c, 3), "device_ms": round(dm, 3), "device_ms_min": round(min(dev_ms), 3), "device_ms_max": round(max(dev_ms), 3),
                "plies_per_s": round(P / (c * 1e-3), 1), "device_plies_per_s": round(P / (dm * 1e-3), 1)}

    rows = {"san_write": timed(lambda: L.sc_moves_to_san_device(0, n, p(mv), p(off), stream, d_tok, st_write))}
    status = download(st_write, n, np.int32)
    if status.any():
        raise SystemExit("san_write: status of %d games is not 0" % np.count_nonzero(status))
    written = download(d_tok, P, np.uint64)
    text = [scamd.san.movetext(written[off[g]:off[g + 1]]) for g in range(n)]
    tokens, toff = scamd.san.pack_tokens(text)
    assert np.array_equal(off, toff), "a game's token count is not its ply count"
    rows["san_moves"] = timed(lambda: L.sc_encode_san_device(None, 0, n, p(tokens), p(toff), 0, 0, stream, None, None, None, None, None, None,
                                                              d_moves, st_parse))
    if download(st_parse, n, np.int32).any() or not np.array_equal(download(d_moves, P, np.uint16), mv):
        raise SystemExit("san_moves: the writer's text does not read back to the moves")
    for q in bufs:
        hip.hipFree(q)
    words = [scamd.san.token_text(t) for t in written]
    line = json.dumps({"tool": "san_write_rate", "host": socket.gethostname(), "date": datetime.date.today().isoformat(), "games": n, "plies": P,
                       "longest": int(np.diff(off.astype(np.int64)).max()), "reps": args.reps, "rows": rows,
                       "write_over_parse_device": round(rows["san_write"]["device_ms"] / rows["san_moves"]["device_ms"], 3),
                       "words": {"check": sum(w.endswith("+") for w in words), "mate": sum(w.endswith("#") for w in words),
                                 "longest": max(len(w) for w in words)}})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
