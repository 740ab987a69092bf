"""The search report restated in plain Python (no device, no library): the ranking of the root's children, the walk of a principal
variation, the end codes, q and the cp / mate scores, over a tree dict with the keys of SelfPlay.tree() / oracle Search.dump()
(n, q = the value SUMS, move, first_child, n_child; prior where the tree has it).

tests/test_report_ref.py holds this file to hand-built trees and tells every rule from a deliberately wrong one;
tests/test_gpu_report.py compares sc_selfplay_report with it bit for bit.

A device tree marks a terminal node in first_child (-2 drawn, -3 White won, -4 Black won: search_expand.hpp); the oracle's dump
leaves -1 there and finds the outcome again on every visit.  Both say the same thing: a node that has been visited and has no
children is a terminal, and its value sum over its visits is the outcome.  header() reads either form."""
import math

import numpy as np

END_OPEN, END_DRAW, END_WHITE_WON, END_BLACK_WON, END_DEPTH = range(5)
MAX_PV = 1024
WHITE, BLACK = 1, 0

# the rules, and for each the wrong variant test_report_ref.py tells it from
RIGHT = dict(tie="first",             # "last": the LAST most-visited child (the descent's own max_by rule, which mcts::step does not use)
             follow_unvisited=False,  # True: the walk steps to a child without a visit
             rank_by="n",             # "w": ranks by the value sum
             walk_limit=MAX_PV,       # 64: one wavefront of moves
             black_flip=True,         # False: q stays White's
             mate_sign="parity")      # "value": the sign of q


def uci(m):
    """the UCI text of a move word (from | to << 6 | promo << 12)"""
    m = int(m)
    sq = lambda s: "abcdefgh"[s & 7] + "12345678"[s >> 3]   # noqa: E731
    return sq(m & 63) + sq((m >> 6) & 63) + ("", "", "n", "b", "r", "q")[(m >> 12) & 7]


def header(t, x):
    """the header of node x: >= 0 its first child, -1 open, -2 / -3 / -4 terminal (drawn / White won / Black won)"""
    fc, nc, n = int(t["first_child"][x]), int(t["n_child"][x]), int(t["n"][x])
    if fc <= -2 or (fc >= 0 and nc > 0):
        return fc
    if n > 0 and nc == 0:   # visited and childless: the outcome is the value of every visit
        w = float(t["q"][x])
        return -2 if w == 0.0 else -3 if w > 0.0 else -4
    return -1


def most_visited(t, fc, nc, rules=RIGHT):
    """(index among the children, its visits): the maximum of N, ties to the lowest index"""
    ns = [int(v) for v in t["n"][fc:fc + nc]]
    top = max(ns)
    idx = ns.index(top) if rules["tie"] == "first" else nc - 1 - ns[::-1].index(top)
    return idx, top


def ranks(t, fc, nc, rules=RIGHT):
    """rank of every root child: #{ j : N[j] > N[i], or N[j] == N[i] and j < i }"""
    key = t["n"] if rules["rank_by"] == "n" else t["q"]
    v = [key[fc + i] for i in range(nc)]
    if rules["tie"] == "first":
        return [sum(1 for j in range(nc) if v[j] > v[i] or (v[j] == v[i] and j < i)) for i in range(nc)]
    return [sum(1 for j in range(nc) if v[j] > v[i] or (v[j] == v[i] and j > i)) for i in range(nc)]


def walk(t, x, rules=RIGHT):
    """the variation from root child x on -> (node indices, end code)"""
    nodes = [x]
    while True:
        h = header(t, x)
        if h <= -2:
            return nodes, {-2: END_DRAW, -3: END_WHITE_WON, -4: END_BLACK_WON}[h]
        nc = int(t["n_child"][x])
        if h < 0 or nc == 0:
            return nodes, END_OPEN
        idx, top = most_visited(t, h, nc, rules)
        if top == 0 and not rules["follow_unvisited"]:
            return nodes, END_OPEN
        if len(nodes) >= rules["walk_limit"]:
            return nodes, END_DEPTH
        x = h + idx
        nodes.append(x)


def line_q(w, n, turn, rules=RIGHT):
    """float32 W / N for the side to move at the root; 0 without a visit"""
    if n == 0:
        return np.float32(0.0)
    q = np.float32(w) / np.float32(n)
    return -q if rules["black_flip"] and turn == BLACK else q


def centipawns(q):
    s = min(max((float(q) + 1.0) / 2.0, 0.001), 0.999)
    return int(round(400.0 * math.log10(s / (1.0 - s))))


def score(q, length, end, rules=RIGHT):
    if end in (END_WHITE_WON, END_BLACK_WON):
        m = (length + 1) // 2 if length & 1 else length // 2
        if rules["mate_sign"] == "parity":
            return ("mate", m if length & 1 else -m)
        return ("mate", m if q > 0 else -m)
    return ("cp", centipawns(q))


def allocate_ms(remaining, inc, movestogo):
    """the engine's time for one move: remaining / max(movestogo, 30) + inc / 2, at most half the remaining time"""
    return min(remaining / max(movestogo, 30) + inc / 2, remaining / 2)


def report(t, turn, multipv=1, pv_cap=64, live=True, rules=RIGHT):
    """What sc_selfplay_report says of one slot whose tree is t and whose root has `turn` to move; live: the slot is active and has
    searched.  -> dict(n_nodes, n_root_children, root_children_n, root_n, root_w, n_lines, lines=[dict(child, n, w, prior, len, end,
    moves (the first min(len, pv_cap) move words), pv (the same as UCI), move, q, score)])"""
    n_nodes = len(t["n"])
    out = dict(n_nodes=n_nodes, n_root_children=0, root_children_n=0, root_n=0, root_w=np.float32(0), n_lines=0, lines=[])
    if n_nodes == 0:
        return out
    out.update(root_n=int(t["n"][0]), root_w=np.float32(t["q"][0]))
    fc, nc = int(t["first_child"][0]), int(t["n_child"][0])
    if fc < 0 or nc == 0:
        return out
    out.update(n_root_children=nc, root_children_n=int(sum(int(v) for v in t["n"][fc:fc + nc])))
    if not live:
        return out
    rk = ranks(t, fc, nc, rules)
    out["n_lines"] = min(multipv, nc)
    for r in range(out["n_lines"]):
        child = rk.index(r)
        x = fc + child
        nodes, end = walk(t, x, rules)
        n, w = int(t["n"][x]), np.float32(t["q"][x])
        q = line_q(w, n, turn, rules)
        moves = [int(t["move"][y]) for y in nodes[:pv_cap]]
        out["lines"].append(dict(child=child, n=n, w=w, prior=np.float32(t["prior"][x]) if "prior" in t else None, len=len(nodes), end=end,
                                 moves=moves, pv=[uci(m) for m in moves], move=uci(t["move"][x]), q=float(q), score=score(q, len(nodes), end, rules)))
    return out


def make_tree(nodes):
    """a tree dict from a list of (n, w, move, first_child, n_child) rows (priors: 1 / 16 each)"""
    a = np.asarray([r[:2] for r in nodes], np.float64).reshape(-1, 2)
    return dict(n=a[:, 0].astype(np.int32), q=a[:, 1].astype(np.float32), move=np.asarray([r[2] for r in nodes], np.uint16),
                first_child=np.asarray([r[3] for r in nodes], np.int32), n_child=np.asarray([r[4] for r in nodes], np.int32),
                prior=np.full(len(nodes), 1.0 / 16, np.float32))


class StubSearcher:
    """the searcher a scamd.uci.Protocol drives, without a device: every run() of k simulations adds k visits; the report names
    `moves[j]` as line j + 1 with fixed statistics.  on_run(searcher): called at the start of every run (a test posts `stop` from it)."""

    def __init__(self, moves=("e2e4", "d2d4", "g1f3"), flags_at=None, on_run=None, mate=None):
        self.moves, self.flags_at, self.on_run, self.mate = list(moves), flags_at, on_run, mate
        self.sim, self.calls, self.position, self.cpuct, self.runs = 0, [], None, None, []

    def new_game(self):
        self.calls.append("new_game")

    def set_position(self, fen, moves):
        self.position = (fen, list(moves))

    def start(self, cpuct):
        self.cpuct, self.sim, self.runs = cpuct, 0, []

    def run(self, n):
        if self.on_run:
            self.on_run(self)
        self.runs.append(n)
        self.sim += n
        return 8 if self.flags_at is not None and self.sim >= self.flags_at else 0

    def report(self, multipv):
        lines = []
        for j, mv in enumerate(self.moves[:multipv]):
            pv = [mv, "e7e5"][:2 - j % 2]
            sc = ("mate", self.mate) if self.mate is not None and j == 0 else ("cp", 30 - 10 * j)
            lines.append(dict(move=mv, pv=pv, n=self.sim // (j + 1), q=0.1, prior=0.1, len=len(pv), end=0, score=sc))
        return dict(sim=self.sim, lines=lines)

    def close(self):
        self.calls.append("close")
