"""Rate of reading SAN game records on the device (sc_encode_san_device: parse + encode in one call) against its floor, the same
encoder without the parse (sc_encode_steps_device on the same games given as moves and children), on the 256-game trace set of
tools/ratelib.py rendered to SAN.  Prints one JSON line and appends it to profiles/san_rate_<date>.jsonl (--out).

  python tools/san_rate.py [--reps 7] [--out FILE]

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
import time

import numpy as np

from ratelib import Hip, common_args, emit, ptr as p, record, require_device, spread, trace_set  # sets the package path

import scamd  # noqa: E402
import scamd.san  # noqa: E402


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
    common_args(ap, reps=7)
    ap.add_argument("--out", default=None, help="result file (default profiles/san_rate_<date>.jsonl)")
    args = ap.parse_args()
    L = require_device()
    eng = scamd.Engine(args.blocks, args.channels, seed=1)
    games = trace_set(eng)
    eng.close()
    hip = Hip(L)
    alloc, download, stream = hip.alloc, hip.download, hip.stream

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
        call_ms, _, dev_ms = hip.timed(call, args.reps)
        c, (dm, lo, hi) = spread(call_ms)[0], spread(dev_ms)
        rows[name] = {"call_ms": round(c, 3), "device_ms": round(dm, 3), "device_ms_min": round(lo, 3), "device_ms_max": round(hi, 3),
                      "plies_per_s": round(P / (c * 1e-3), 1), "device_plies_per_s": round(P / (dm * 1e-3), 1)}
        status = download(st_steps if name == "steps_legal" else st_san, n, np.int32)
        if status.any():
            bad = np.nonzero(status)[0]
            raise SystemExit(f"{name}: status of {bad.size} games is not 0, e.g. {[(int(g), int(status[g])) for g in bad[:8]]}")
        if name.startswith("san") and not np.array_equal(download(d_moves, P, np.uint16), mv[:P]):
            raise SystemExit(f"{name}: the parsed moves are not the traces' moves")
    if not np.array_equal(download(dl_san, (P, 224), np.uint32), download(dl_steps, (P, 224), np.uint32)):
        raise SystemExit("dist_legal differs between the SAN path and the moves-and-children path")
    hip.close()
    emit([record("san_rate", games=n, plies=P, reps=args.reps, rows=rows,
                 san_over_steps_device=round(rows["san_legal"]["device_ms"] / rows["steps_legal"]["device_ms"], 3),
                 host_prepare={"render_ms": round((t1 - t0) * 1e3, 1), "tokenize_ms": round(tokenize_ms, 1), "token_bytes": int(tokens.nbytes),
                               "moves_and_children_bytes": int(mv.nbytes + cm.nbytes + cn.nbytes + coff.nbytes)})], args.out, "san_rate")


if __name__ == "__main__":
    main()
