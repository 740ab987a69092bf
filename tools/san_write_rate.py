"""Rate of writing SAN on the device (sc_moves_to_san_device: walk + one wavefront per ply) next to reading it back
(sc_encode_san_device with only moves + status: the parser's latency chain), on the 256-game trace set of
tools/ratelib.py.  Prints one JSON line and appends it to profiles/san_write_rate_<date>.jsonl (--out).

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

import numpy as np

from ratelib import Hip, common_args, emit, ptr as p, record, require_device, spread, trace_set  # sets the package path

import scamd  # noqa: E402
import scamd.san  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    common_args(ap, reps=7)
    ap.add_argument("--out", default=None, help="result file (default profiles/san_write_rate_<date>.jsonl)")
    args = ap.parse_args()
    L = require_device()
    eng = scamd.Engine(args.blocks, args.channels, seed=1)
    games = trace_set(eng)
    eng.close()
    hip = Hip(L)
    alloc, download, stream = hip.alloc, hip.download, hip.stream

    mv = np.asarray([scamd.uci_move(s[0]) if isinstance(s[0], str) else int(s[0]) for g in games for s in g], np.uint16)
    off = np.zeros(len(games) + 1, np.uint32)
    off[1:] = np.cumsum([len(g) for g in games])
    n, P = len(games), int(off[-1])
    d_tok, d_moves, st_write, st_parse = alloc(P * 8), alloc(P * 2), alloc(n * 4), alloc(n * 4)

    def row_of(call):
        call_ms, _, dev_ms = hip.timed(call, args.reps)
        c, (dm, lo, hi) = spread(call_ms)[0], spread(dev_ms)
        return {"call_ms": round(c, 3), "device_ms": round(dm, 3), "device_ms_min": round(lo, 3), "device_ms_max": round(hi, 3),
                "plies_per_s": round(P / (c * 1e-3), 1), "device_plies_per_s": round(P / (dm * 1e-3), 1)}

    rows = {"san_write": row_of(lambda: L.sc_moves_to_san_device(0, n, p(mv), p(off), stream, d_tok, st_write))}
    status = download(st_write, n, np.int32)
    if status.any():
        raise SystemExit("san_write: status of %d games is not 0" % np.count_nonzero(status))
    written = download(d_tok, P, np.uint64)
    text = [scamd.san.movetext(written[off[g]:off[g + 1]]) for g in range(n)]
    tokens, toff = scamd.san.pack_tokens(text)
    assert np.array_equal(off, toff), "a game's token count is not its ply count"
    rows["san_moves"] = row_of(lambda: L.sc_encode_san_device(None, 0, n, p(tokens), p(toff), 0, 0, stream, None, None, None, None, None, None,
                                                              d_moves, st_parse))
    if download(st_parse, n, np.int32).any() or not np.array_equal(download(d_moves, P, np.uint16), mv):
        raise SystemExit("san_moves: the writer's text does not read back to the moves")
    hip.close()
    words = [scamd.san.token_text(t) for t in written]
    emit([record("san_write_rate", games=n, plies=P, longest=int(np.diff(off.astype(np.int64)).max()), reps=args.reps, rows=rows,
                 write_over_parse_device=round(rows["san_write"]["device_ms"] / rows["san_moves"]["device_ms"], 3),
                 words={"check": sum(w.endswith("+") for w in words), "mate": sum(w.endswith("#") for w in words),
                        "longest": max(len(w) for w in words)})], args.out, "san_write_rate")


if __name__ == "__main__":
    main()
