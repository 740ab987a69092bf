"""perft of a position on the GPU (scamd.rules.perft, sc_perft): the divide as other engines print it -- one `move: count` line per
legal move in the generator's order, a blank line, the total -- and with --kinds the counts of the last moves' kinds.

  python tools/perft.py --depth 5
  python tools/perft.py --fen "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1" --depth 4 --kinds
  python tools/perft.py --moves e2e4 e7e5 --depth 4

The position is --fen (default: the start position) followed by --moves (UCI)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smart-chess-rust_amd"))

from scamd import rules  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--fen", default=None, help="the base position (default: the start position)")
    ap.add_argument("--moves", nargs="*", default=[], help="UCI moves played from the base")
    ap.add_argument("--depth", type=int, required=True)
    ap.add_argument("--kinds", action="store_true", help="also captures, en passant, castles, promotions, checks, checkmates")
    ap.add_argument("--max-frontier", type=int, default=0, help="node records per level buffer (0: the library's default)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    r = rules.perft([args.moves], args.depth, fens=None if args.fen is None else [args.fen], device=args.device, divide=True,
                    kinds=args.kinds, max_frontier=args.max_frontier)
    if r["status"][0]:
        raise SystemExit(f"move {-int(r['status'][0]) - 1} of --moves ({args.moves[-int(r['status'][0]) - 1]}) is not legal")
    for uci, count in r["divide"][0]:
        print(f"{uci}: {count}")
    print()
    print(f"Nodes searched: {int(r['nodes'][0])}")
    if args.kinds:
        for name in rules.KINDS:
            print(f"{name}: {int(r['kinds'][name][0])}")


if __name__ == "__main__":
    main()
