"""A stub UCI engine for the tests of scamd.external.UciOpponent: it answers `go` from a table {position line: move} and knows no
chess.  python uci_stub.py --table T.json [--log FILE] [--delay S] [--die-after N] [--none] [--default MOVE]
  --log       every line received is appended to FILE (one file per process: the pid is put in front of the extension)
  --delay     seconds to sleep before every bestmove
  --die-after exit without an answer at go number N + 1
  --none      answer `bestmove (none)`
  --default   the answer to a position the table does not hold (else `bestmove 0000`)"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table")
    ap.add_argument("--log")
    ap.add_argument("--delay", type=float, default=0.0)
    ap.add_argument("--die-after", type=int, default=-1)
    ap.add_argument("--none", action="store_true")
    ap.add_argument("--default", default="0000")
    a = ap.parse_args()
    table = json.load(open(a.table)) if a.table else {}
    log = None
    if a.log:
        root, extn = os.path.splitext(a.log)
        log = open(f"{root}.{os.getpid()}{extn}", "a")
    position, n_go = "", 0

    def say(text):
        sys.stdout.write(text + "\n")
        sys.stdout.flush()

    for raw in sys.stdin:
        line = raw.strip()
        if log:
            log.write(line + "\n")
            log.flush()
        word = line.split(" ", 1)[0] if line else ""
        if word == "uci":
            say("id name uci_stub")
            say("option name Skill Level type spin default 20 min 0 max 20")
            say("uciok")
        elif word == "isready":
            say("readyok")
        elif word == "position":
            position = line
        elif word == "go":
            if a.die_after >= 0 and n_go >= a.die_after:
                sys.exit(3)
            n_go += 1
            if a.delay:
                time.sleep(a.delay)
            say("info depth 1 score cp 0")
            say("bestmove " + ("(none)" if a.none else table.get(position, a.default)))
        elif word == "quit":
            break
    if log:
        log.close()


if __name__ == "__main__":
    main()
