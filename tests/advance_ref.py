"""What the advance tests share (sc_selfplay_advance: a move is played and the searched subtree below it is kept):
  reroot            the re-rooting of a dumped tree in numpy: the ascending mark sweep and the stable compaction
  same_first_child  a device tree's first_child against the oracle's
  oracle_after      the oracle's search of a position after s simulations
  KeepStub          the searcher a scamd.uci.Protocol drives without a device, one that can keep its tree
Nothing here touches the package or the device."""
import numpy as np

import deep_lines as dl


def reroot(tree, child):
    """`tree` (arrays per node: n, q, uct, move, first_child, n_child and whatever else a dump holds) with node `child` as
    its root.  A node's child block lies behind the node, so one ascending sweep from `child` that marks [fc, fc + nc) of every
    marked node finds the subtree; a kept node's new index is the number of kept nodes in front of it.  The new root has
    uct 0 (and prior 0, parent -1) as a fresh root has; its move is left alone (no comparison reads a root's move)."""
    fc, nc = tree["first_child"], tree["n_child"]
    n = len(fc)
    keep = np.zeros(n, bool)
    keep[child] = True
    for i in range(child, n):
        if keep[i] and fc[i] >= 0 and nc[i] > 0:
            assert fc[i] > i and fc[i] + nc[i] <= n, i
            keep[fc[i]:fc[i] + nc[i]] = True
    new = np.cumsum(keep) - 1
    out = {k: np.asarray(v)[keep].copy() for k, v in tree.items()}
    f = out["first_child"]
    f[f >= 0] = new[f[f >= 0]]
    if "parent" in out:
        out["parent"] = np.where(np.flatnonzero(keep) == child, -1, new[np.maximum(tree["parent"][keep], 0)]).astype(np.int32)
    out["uct"][0] = 0
    if "prior" in out:
        out["prior"][0] = 0
    return out


def same_first_child(t, d):
    """first_child of a device tree t (or of a rerooted dump) against the oracle's dump d, which has -1 for every node without
    children where the device tells unexpanded (-1) from terminal (-2, -3, -4)"""
    a, b = np.asarray(t["first_child"]), np.asarray(d["first_child"])
    return len(a) == len(b) and np.array_equal(np.where(a >= 0, a, -1), np.where(b >= 0, b, -1))


def oracle_after(orc, state, sims, evaluator="synth", cpuct=2.5):
    """the oracle's Search of `state` after `sims` simulations, no noise"""
    srch = orc.Search(state)
    for _ in range(sims):
        srch.sim(evaluator=dl.EVALUATORS[evaluator], cpuct=cpuct, with_noise=False)
    return srch


class KeepStub:
    """a searcher with advance(): every run() of k simulations adds k visits to the tree it holds; advance(move) keeps a third of
    them, or refuses the moves in `refuse`.  log: the calls, in order"""

    def __init__(self, refuse=()):
        self.refuse, self.log, self.visits, self.sim = set(refuse), [], 0, 0

    def new_game(self):
        self.log.append(("new_game",))

    def set_position(self, fen, moves):
        self.log.append(("set_position", fen, list(moves)))

    def advance(self, move):
        if move in self.refuse:
            self.log.append(("refused", move))
            return None
        self.visits //= 3
        self.log.append(("advance", move, self.visits))
        return 7 * self.visits + 1, self.visits

    def start(self, cpuct, live=False):
        self.log.append(("start", live))
        self.sim = 0
        if not live:
            self.visits = 0

    def run(self, n):
        self.sim += n
        self.visits += n
        return 0

    def report(self, multipv):
        return dict(sim=self.sim, lines=[dict(move="e2e4", pv=["e2e4"], n=self.visits, q=0.1, prior=0.1, len=1, end=0, score=("cp", 10))])

    def close(self):
        self.log.append(("close",))
