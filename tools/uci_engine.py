"""The engine as a UCI program: open it in a GUI, pair it in a tournament manager, or hand it to tools/play_uci.py as the opponent.

  python tools/uci_engine.py -w net.scw [--fp8] [--evaluator net|synth|synth_coarse|synth_uniform] [--salt S] [--device N]
                             [--blocks B --channels C --net-seed S]     (a random network when no weights are given)
                             [--keep-tree]                              (the option KeepTree starts as true)

Options over the protocol: MultiPV, CPuct, Chunk (simulations between two looks at the input and the clock), InfoEvery (ms).
Every `go` searches from a fresh tree; `go nodes N` is one sc_search of N simulations (scamd/uci.py).  With KeepTree (a check
option; --keep-tree sets it from the start) a `position` that extends the current game keeps the searched subtree below the moves
played, and `go nodes N` runs N more simulations on it.  The synthetic evaluators need no network: they exist for tests.

The reader thread is started FIRST and the GPU is opened after it: no HIP call precedes the thread's start, and the program starts
no child process."""
import argparse
import os
import queue
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smart-chess-rust_amd"))


def reader(q, stream):
    """stdin -> queue, one line each; None at the end of input"""
    for line in stream:
        q.put(line.rstrip("\r\n"))
    q.put(None)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-w", "--weights", default=None, help="an .scw blob (tools/ckpt_to_scw.py)")
    ap.add_argument("--fp8", action="store_true", help="the fp8 tower")
    ap.add_argument("--evaluator", default="net", choices=["net", "synth", "synth_coarse", "synth_uniform"])
    ap.add_argument("--salt", type=lambda s: int(s, 0), default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--net-seed", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--keep-tree", action="store_true", help="start with the option KeepTree set")
    a = ap.parse_args()

    q = queue.Queue()
    threading.Thread(target=reader, args=(q, sys.stdin), daemon=True).start()

    def write(text):
        sys.stdout.write(text + "\n")
        sys.stdout.flush()

    # the GPU is opened from here on
    import scamd
    from scamd import uci
    if scamd.lib().sc_device_count() <= 0:
        write("info string no HIP device: the engine has no CPU fallback")
        return 1
    eng = None
    if a.evaluator == "net":
        eng = scamd.Engine(a.blocks, a.channels, seed=a.net_seed, weights=a.weights, precision="fp8" if a.fp8 else "bf16", device=a.device)
    searcher = uci.LibSearcher(eng, evaluator=a.evaluator, salt=a.salt, seed=a.seed, device=a.device)
    proto = uci.Protocol(searcher, write)
    proto.opt["KeepTree"] = a.keep_tree
    rc = proto.run(q)
    if eng is not None:
        eng.close()
    return rc


if __name__ == "__main__":
    sys.exit(main())
