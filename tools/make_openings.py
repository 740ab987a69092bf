"""Opening suites for evaluation matches (sc-play --openings, scamd.play_match(openings=...), SelfPlay.set_openings): every legal
line of P plies from the start position, in move-generation order, one line of UCI moves per opening.  The moves come from the
GPU rules (scamd.encode_positions), so the tool needs a GPU.  1, 2 and 3 plies give 20, 400 and 8 902 lines (perft); a line whose
last position ends the game (possible from 4 plies on) cannot open a game and is left out.

    python tools/make_openings.py --plies 2 [--out openings_2.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smart-chess-rust_amd"))
import scamd  # noqa: E402

CHUNK = 4096   # positions per sc_encode_positions call


def generate(plies):
    """-> (lines, dropped): the lines of `plies` plies as lists of UCI strings; dropped = lines that end the game"""
    lines = [[]]
    for _ in range(plies):
        nxt = []
        for i in range(0, len(lines), CHUNK):
            part = lines[i:i + CHUNK]
            enc = scamd.encode_positions(part)
            for ln, moves in zip(part, enc["legal_moves"]):
                nxt.extend(ln + [scamd.move_uci(m)] for m in moves)
        lines = nxt
    keep = []
    for i in range(0, len(lines), CHUNK):
        part = lines[i:i + CHUNK]
        enc = scamd.encode_positions(part)
        keep.extend(ln for ln, term, n in zip(part, enc["termination"], enc["n_legal"]) if term == 0 and n > 0)
    return keep, len(lines) - len(keep)


def write(path, lines):
    with open(path, "w") as f:
        for ln in lines:
            f.write(" ".join(ln) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--plies", type=int, required=True)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not 0 <= args.plies <= 4:
        raise SystemExit("--plies must be 0..4 (5 plies are 4 865 609 lines)")
    if scamd.lib().sc_device_count() <= 0:
        raise SystemExit("no HIP device")
    lines, dropped = generate(args.plies)
    out = args.out or f"openings_{args.plies}.txt"
    write(out, lines)
    print(f"{len(lines)} lines of {args.plies} plies -> {out}" + (f" ({dropped} end the game: left out)" if dropped else ""))


if __name__ == "__main__":
    main()
