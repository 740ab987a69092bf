"""Rate of perft on the device: nodes per second of sc_perft (csrc/perft_kernels.hip, csrc/perft.hip) on the start position at depth
6 and on Kiwipete at depth 5, with and without kinds, at max_frontier 2^16, 2^20 and 2^22, next to the host build of the same
rules code (lib/libsc_rules_host.so, sct_perft) on one core in the same process.  Prints one JSON line per row and appends it to
profiles/perft_rate_<date>.jsonl as soon as the row is measured.

  python tools/perft_rate.py [--reps 5] [--no-baseline]

Every device figure is the median of the wall time of --reps calls after one warm-up call, with the smallest and the largest next
to it (ms_min / ms_max); a call is synchronous and allocates and frees its own workspace, so the wall time is what a caller
waits.  kernels_ms is sc_perft_last_timing's HIP-event time of the call's launches (median over the same calls), outside_share
the part of the wall time that is not that: allocations, the host's reads of the level totals, copies.  generations is the number
of positions whose moves the walk generates: every node above the last level twice (counted, then expanded), the nodes of depth
`depth` - 1 once; with kinds also once per last move that gives check.  The node totals are compared with the published values
before anything is timed.  No torch in the process."""
import argparse
import ctypes as C
import os
import time

from ratelib import ROOT, emit, record, require_device, spread  # sets the package path

from scamd import rules  # noqa: E402

START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
KIWI = "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1"
CASES = (("startpos", START, 6, 119060324), ("kiwipete", KIWI, 5, 193690690))
FRONTIERS = (1 << 16, 1 << 20, 1 << 22)


def host_rules():
    H = C.CDLL(os.path.join(ROOT, "smart-chess-rust_amd", "lib", "libsc_rules_host.so"))
    H.sct_new.restype = C.c_void_p
    H.sct_free.argtypes = [C.c_void_p]
    H.sct_set_fen.argtypes = [C.c_void_p, C.c_char_p]
    H.sct_perft.restype = C.c_uint64
    H.sct_perft.argtypes = [C.c_void_p, C.c_int]
    return H


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true", help="skip the host rows (tens of seconds of one core)")
    ap.add_argument("--out", default=None, help="result file (default profiles/perft_rate_<date>.jsonl)")
    args = ap.parse_args()
    require_device()
    base = record("perft_rate", reps=args.reps)
    for name, fen, depth, want in CASES:
        # the levels' sizes (one divide-free call per depth): what the walk generates
        level = [int(rules.perft([[]], d, fens=[fen])["nodes"][0]) for d in range(depth)]
        checks = int(rules.perft([[]], depth, fens=[fen], kinds=True)["kinds"]["checks"][0])
        gens = 2 * sum(level[:-1]) + level[-1]
        for with_kinds in (False, True):
            for frontier in FRONTIERS:
                wall, kern = [], []
                for rep in range(args.reps + 1):
                    t0 = time.perf_counter()
                    r = rules.perft([[]], depth, fens=[fen], kinds=with_kinds, max_frontier=frontier)
                    t1 = time.perf_counter()
                    assert int(r["nodes"][0]) == want and int(r["status"][0]) == 0, (name, r["nodes"])
                    if rep:   # the first call is the warm-up
                        wall.append((t1 - t0) * 1e3)
                        kern.append(rules.last_timing()[0])
                (ms, lo, hi), k_ms = spread(wall), spread(kern)[0]
                g = gens + (checks if with_kinds else 0)
                emit([dict(base, row="sc_perft", position=name, depth=depth, nodes=want, kinds=with_kinds, max_frontier=frontier,
                           ms=round(ms, 3), ms_min=round(lo, 3), ms_max=round(hi, 3), nodes_per_s=round(want / (ms * 1e-3), 1),
                           kernels_ms=round(k_ms, 3), outside_share=round(1 - k_ms / ms, 4), generations=g,
                           ns_per_generation=round(k_ms * 1e6 / g, 2))], args.out, "perft_rate")
        if not args.no_baseline:
            H = host_rules()
            s = C.c_void_p(H.sct_new())
            assert H.sct_set_fen(s, fen.encode()) == 0
            t0 = time.perf_counter()
            got = int(H.sct_perft(s, depth))
            ms = (time.perf_counter() - t0) * 1e3
            H.sct_free(s)
            assert got == want, (name, got)
            emit([dict(base, row="host_sct_perft_one_core", position=name, depth=depth, nodes=want, ms=round(ms, 1),
                       nodes_per_s=round(want / (ms * 1e-3), 1), runs=1)], args.out, "perft_rate")


if __name__ == "__main__":
    main()
