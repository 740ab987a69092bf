"""Rate of reading SAN game records on the device (sc_encode_san_device: parse + encode in one call) against its floor, the same
encoder without the parse (sc_encode_steps_device on the same games given as moves and children), on the 256-game trace set of
tools/encode_device_rate.py rendered to SAN.  Prints one JSON line.

  python tools/san_rate.py [--reps 7]

rows, all with the reference layout (int8 planes) and dist="legal":
  san_legal     sc_encode_san_device, every output but the dense dist
  steps_legal   sc_encode_steps_device, the same outputs, children = the legal moves with count 1 on the move played
  san_moves     sc_encode_san_device with only moves + status: the tokens' upload and the parser kernel alone
  device_ms     HIP events recorded on the caller's stream around the call;  call_ms: host wall time of the call plus the wait
                for its stream.  Medians over --reps regions after one warm-up call; the inputs are tokenized / packed and the
                output buffers allocated once, outside the timing.
The SAN is written fully specified ("Ng1-f3", "e7xd8=Q", "O-O"): that needs the moving piece only, which a mailbox board here
tracks -- the rules stay on the GPU.  The parsed moves must be the traces' moves, and both paths' dist_legal rows the same bits."""
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


def _sq(s):
    return "abcdefgh"[s & 7] + str((s >> 3) + 1)


def render_san(uci_moves):
    """a game's UCI moves from the start position -> fully specified SAN movetext"""
    back = "RNBQKBNR"
    board = {}
    for f in range(8):
        board[f], board[8 + f], board[48 + f], board[56 + f] = back[f], "P", "P", back[f]
    words = []
    for i, u in enumerate(uci_moves):
        m = scamd.uci_move(u) if isinstance(u, str) else int(u)
        fr, to, promo = m & 63, (m >> 6) & 63, m >> 12
        pc = board.pop(fr)
        cap = to in board
        if pc == "P" and (fr & 7) != (to & 7) and not cap:   # en passant
            del board[(fr & 56) | (to & 7)]
            cap = True
        if pc == "K" and abs(to - fr) == 2:
            rook_from, rook_to = ((fr & 56) | 7, to - 1) if to > fr else (fr & 56, to + 1)
            board[rook_to] = board.pop(rook_from)
            w = "O-O" if to > fr else "O-O-O"
        else:
            w = ("" if pc == "P" else pc) + _sq(fr) + ("x" if cap else "-") + _sq(to) + ("=" + " NBRQ"[promo - 1] if promo else "")
        board[to] = " NBRQ"[promo - 1] if promo else pc
        words.append(("%d. " % (i // 2 + 1) if i % 2 == 0 else "") + w)
    return " ".join(words)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--channels", type=int, default=128)
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

    t0 = time.perf_counter()
    text = [render_san([s[0] for s in g]) for g in games]
    t1 = time.perf_counter()
    tokens, toff = scamd.san.pack_tokens(text)
    tokenize_ms = (time.perf_counter() - t1) * 1e3
    one_hot = [[(s[0], [(c[0], 1 if c[0] == s[0] else 0) for c in s[1]]) for s in g] for g in games]
    mv, off, cm, cn, coff = scamd.pack_steps(one_hot)
    n, P = len(games), int(off[-1])
    assert np.array_equal(off, toff), "a game's token count is not its ply count"
    boards, meta, lidx, nl = alloc(P * 7168), alloc(P * 28), alloc(P * 448), alloc(P * 4)
    dl_san, dl_steps, d_moves = alloc(P * 224 * 4), alloc(P * 224 * 4), alloc(P * 2)
    st_san, st_steps = alloc(n * 4), alloc(n * 4)
    calls = {
        "san_legal": lambda: L.sc_encode_san_device(None, 0, n, p(tokens), p(toff), 0, 0, stream, boards, meta, None, dl_san, lidx, nl, d_moves, st_san),
        "steps_legal": lambda: L.sc_encode_steps_device(None, 0, n, p(mv), p(off), p(cm), p(cn), p(coff), 0, 0, stream, boards, meta, None, dl_steps,
                                                        lidx, nl, st_steps),
        "san_moves": lambda: L.sc_encode_san_device(None, 0, n, p(tokens), p(toff), 0, 0, stream, None, None, None, None, None, None, d_moves, st_san),
    }
    rows = {}
    for name, call in calls.items():
        def checked():
            rc = call()
            assert rc == 0, L.sc_last_error().decode()
        checked()
        assert hip.hipStreamSynchronize(stream) == 0
        call_ms, dev_ms = [], []
        for _ in range(args.reps):
            t0_ = time.perf_counter()
            hip.hipEventRecord(e0, stream)
            checked()
            hip.hipEventRecord(e1, stream)
            assert hip.hipStreamSynchronize(stream) == 0
            call_ms.append((time.perf_counter() - t0_) * 1e3)
            ms = C.c_float(0)
            hip.hipEventElapsedTime(C.byref(ms), e0, e1)
            dev_ms.append(ms.value)
        c, dm = statistics.median(call_ms), statistics.median(dev_ms)
        rows[name] = {"call_ms": round(c, 3), "device_ms": round(dm, 3), "device_ms_min": round(min(dev_ms), 3), "device_ms_max": round(max(dev_ms), 3),
                      "plies_per_s": round(P / (c * 1e-3), 1), "device_plies_per_s": round(P / (dm * 1e-3), 1)}
        status = download(st_steps if name == "steps_legal" else st_san, n, np.int32)
        if status.any():
            bad = np.nonzero(status)[0]
            raise SystemExit(f"{name}: status of {bad.size} games is not 0, e.g. {[(int(g), int(status[g])) for g in bad[:8]]}")
        if name.startswith("san") and not np.array_equal(download(d_moves, P, np.uint16), mv[:P]):
            raise SystemExit(f"{name}: the parsed moves are not the traces' moves")
    if not np.array_equal(download(dl_san, (P, 224), np.uint32), download(dl_steps, (P, 224), np.uint32)):
        raise SystemExit("dist_legal differs between the SAN path and the moves-and-children path")
    for q in bufs:
        hip.hipFree(q)
    print(json.dumps({"tool": "san_rate", "host": socket.gethostname(), "date": datetime.date.today().isoformat(), "games": n, "plies": P,
                      "reps": args.reps, "rows": rows,
                      "san_over_steps_device": round(rows["san_legal"]["device_ms"] / rows["steps_legal"]["device_ms"], 3),
                      "host_prepare": {"render_ms": round((t1 - t0) * 1e3, 1), "tokenize_ms": round(tokenize_ms, 1),
                                       "token_bytes": int(tokens.nbytes), "moves_and_children_bytes": int(mv.nbytes + cm.nbytes + cn.nbytes + coff.nbytes)}}))


if __name__ == "__main__":
    main()
