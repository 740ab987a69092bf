"""Trace JSON files already on disk -> one PGN file (needs the GPU: SAN is rendered there, scamd.san.moves_to_san).

    python tools/trace_to_pgn.py -t 'replay/w_*.json' -o games.pgn [--white NAME] [--black NAME] [--event TEXT] [--device 0]

A trace is the reference's {"outcome", "steps"} (steps[i][0] is the UCI move played), with the launchers' optional "opening" (the
UCI moves the game started with) and "fen" (the position it started from).  Files are taken in natural order of their names
(w_2 before w_10) and written as Round 1, 2, ...; Result and Termination come from "outcome"."""
import argparse
import glob
import json
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "smart-chess-rust_amd"))

RESULT = {"White": "1-0", "Black": "0-1", None: "1/2-1/2"}


def natural(name):
    return [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", name)]


def read_trace(path):
    """-> (UCI moves, FEN or None, result or None, termination or None)"""
    js = json.load(open(path))
    moves = list(js.get("opening", [])) + [s[0] for s in js["steps"]]
    oc = js.get("outcome")
    return moves, js.get("fen"), RESULT[oc["winner"]] if oc else None, oc["termination"] if oc else None


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-t", "--traces", required=True, help="glob pattern of the trace files")
    ap.add_argument("-o", "--output", required=True)
    ap.add_argument("--white", default="?")
    ap.add_argument("--black", default="?")
    ap.add_argument("--event", default="?")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    paths = sorted(glob.glob(a.traces), key=natural)
    if not paths:
        ap.error("no file matches " + a.traces)
    import torch  # noqa: F401  (first: libsc_engine.so then binds to the HIP runtime torch loaded)
    import scamd.san as san
    traces = [read_trace(p) for p in paths]
    fens = [t[1] for t in traces]
    sans, status = san.moves_to_san([t[0] for t in traces], fens=fens if any(fens) else None, device=a.device)
    for p, st in zip(paths, status):
        if st:
            sys.exit("%s: move %d is not legal" % (p, -int(st) - 1))
    headers = [dict({"Event": a.event, "Round": k + 1, "White": a.white, "Black": a.black}, **({"Termination": t[3]} if t[3] else {}))
               for k, t in enumerate(traces)]
    san.write_pgn(a.output, sans, results=[t[2] for t in traces], headers=headers, fens=fens)
    print("%d games -> %s" % (len(paths), a.output))


if __name__ == "__main__":
    main()
