"""Cost of the search report (sc_selfplay_report: one launch, one copy for every slot) next to the path it replaces -- one
SelfPlay.tree() per slot and numpy's argmax, as scamd.fen.analyse did it -- and next to one searched ply of the same handle.  Prints
one JSON line per MultiPV setting and appends them to profiles/report_rate_<date>.jsonl (--out).

  python tools/report_rate.py [--slots 256] [--rollout 180] [--multipv 1,8] [--pv-cap 64] [--reps 5] [--out FILE]

Synthetic evaluator (no weights), every slot `rollout` - 1 simulations into a ply of its own self-play game (root noise on: the
games, and so the trees, differ).  Per line, as [median, min, max] over --reps:
  call_ms     host wall time of one SelfPlay-level report call with its numpy arrays (the handle is idle: the wait is for the kernel and the copy)
  device_ms   the kernel's own time: the library's HIP events around it on the handle's stream (sc_selfplay_report_last_timing)
  total_ms    the library's host clock around the whole C call (the same entry point)
  tree_ms     `slots` SelfPlay.tree() calls and the argmax of the root children's visits, the path of analyse before the report
  search_ply_ms  one searched ply (`rollout` simulations enqueued, then the wait for the stream) on the same handle
The tool checks that both paths name the same move in every slot."""
import argparse
import time

import numpy as np

from ratelib import emit, record, require_device, spread  # sets the package path

import scamd  # noqa: E402
from scamd import report as rp  # noqa: E402


def med(xs):
    return [round(x, 4) for x in spread(xs)]


def tree_moves(sp, n):
    """the per-slot path: the whole tree of every slot to the host, the first most-visited root child by numpy"""
    out = []
    for i in range(n):
        t = sp.tree(i)
        fc, nc = (int(t["first_child"][0]), int(t["n_child"][0])) if t["n"].size and t["first_child"][0] >= 0 else (0, 0)
        out.append(int(t["move"][fc + int(np.argmax(t["n"][fc:fc + nc]))]) if nc else -1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--rollout", type=int, default=180)
    ap.add_argument("--multipv", default="1,8", help="MultiPV settings, comma separated")
    ap.add_argument("--pv-cap", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="result file (default profiles/report_rate_<date>.jsonl)")
    args = ap.parse_args()
    multipvs = [int(x) for x in args.multipv.split(",")]
    L = require_device()
    # one ply to warm up, then the searched plies that are timed; the tree of the ply behind them is what is reported on
    sp = scamd.SelfPlay(None, n_slots=args.slots, n_games=args.slots, rollout_num=args.rollout, num_steps=150, cpuct=2.5, with_noise=True, seed=7,
                        evaluator="synth", outcome_gate=1 << 30)
    search = []
    for k in range(args.reps + 1):
        t0 = time.perf_counter()
        sp.enqueue(args.rollout)
        sp.sync()
        if k:
            search.append((time.perf_counter() - t0) * 1e3)
    sp.enqueue(args.rollout - 1)   # the next ply's tree, one simulation short of its end
    sp.sync()
    tree_ms, want = [], None
    for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        want = tree_moves(sp, args.slots)
        tree_ms.append((time.perf_counter() - t0) * 1e3)
    tree_ms = tree_ms[1:]
    lines = []
    for multipv in multipvs:
        out = rp.report_arrays(args.slots, multipv, args.pv_cap)
        call_ms, kernel_ms, total_ms = [], [], []
        for k in range(args.reps + 1):
            t0 = time.perf_counter()
            rep = rp.report(sp, None, multipv, args.pv_cap, out=out)
            call_ms.append((time.perf_counter() - t0) * 1e3)
            km, tm = rp.last_timing(L)
            kernel_ms.append(km)
            total_ms.append(tm)
        got = [int(rep["pv"][i, 0, 0]) if rep["n_lines"][i] and args.pv_cap else -1 for i in range(args.slots)]
        if args.pv_cap and got != want:
            raise SystemExit(f"the report and the per-slot path name different moves in {sum(a != b for a, b in zip(got, want))} slots")
        c, t = med(call_ms[1:]), med(tree_ms)
        lines.append(record("report_rate", slots=args.slots, rollout=args.rollout, multipv=multipv, pv_cap=args.pv_cap, reps=args.reps,
                            nodes_per_slot=int(np.median(rep["n_nodes"])), mean_pv_len=round(float(rep["line_len"][:, 0].mean()), 2),
                            call_ms=c, device_ms=med(kernel_ms[1:]), total_ms=med(total_ms[1:]), tree_ms=t, search_ply_ms=med(search),
                            x_tree_over_report=round(t[0] / c[0], 2), report_share_of_ply=round(c[0] / spread(search)[0], 5),
                            same_moves=True, error_flags=sp.stats()["error_flags"]))
    sp.close()
    emit(lines, args.out, "report_rate")


if __name__ == "__main__":
    main()
