"""Rate of sc_positions_from_fen: FEN text -> validated records in device memory, for a suite of a few thousand positions.
Prints one JSON line and appends it to profiles/fen_rate_<date>.jsonl (--out).

  python tools/fen_rate.py [--positions 4096] [--reps 7] [--out FILE]

The positions are those of synthetic self-play games (256 slots, one position per slot and ply, read back with
sc_selfplay_get_fen), so they are legal, mostly distinct and spread over openings and middlegames.  call_ms: host wall time of
one sc_positions_from_fen call for all of them -- the host's parse of every text, the upload, k_fen_positions and
k_fen_ep_legal, the download of records and status; the call synchronises.  parse_ms: sc_fen_parse alone over the same texts
(host only).  Medians over --reps regions after one warm-up call, [min, max] beside them."""
import argparse
import ctypes as C
import time

from ratelib import emit, record, require_device, spread  # sets the package path

import scamd  # noqa: E402
import scamd.fen  # noqa: E402


def suite(n):
    """n FENs from synthetic self-play: every slot's position after each ply"""
    slots = 256
    plies = (n + slots - 1) // slots
    sp = scamd.SelfPlay(None, n_slots=slots, n_games=slots, rollout_num=8, num_steps=plies + 1, evaluator="synth", with_noise=False,
                        temperature=1.0, temperature_switch=1000, outcome_gate=1 << 30, seed=3)
    out = []
    for _ in range(plies):
        out += [sp.fen(g) for g in range(slots) if sp.slot(g)["status"] == 1]
        sp.enqueue(8)
    sp.close()
    return out[:n]


def med(xs):
    return [round(x, 4) for x in spread(xs)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="result file (default profiles/fen_rate_<date>.jsonl)")
    args = ap.parse_args()
    require_device()
    fens = suite(args.positions)
    call, parse = [], []
    for r in range(args.reps + 1):
        t0 = time.perf_counter()
        pos = scamd.fen.Positions(fens)
        t1 = time.perf_counter()
        assert (pos.status >= 0).all() and len(pos) == len(fens)
        pos.close()
        f = scamd.fen.FenFields()
        raw = [x.encode() for x in fens]
        t2 = time.perf_counter()
        for x in raw:
            scamd.lib().sc_fen_parse(x, len(x), C.byref(f))
        t3 = time.perf_counter()
        if r:
            call.append((t1 - t0) * 1e3)
            parse.append((t3 - t2) * 1e3)
    m = med(call)
    emit([record("fen_rate", positions=len(fens), distinct=len(set(fens)), reps=args.reps, call_ms=m, positions_per_s=round(len(fens) / (m[0] * 1e-3)),
                 parse_loop_ms=med(parse), note="call_ms includes the Python binding's encoding of the texts; parse_loop_ms is a ctypes loop")],
         args.out, "fen_rate")


if __name__ == "__main__":
    main()
