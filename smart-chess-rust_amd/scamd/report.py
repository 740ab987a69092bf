"""The search report (csrc/report.hip, csrc/report_kernels.hip: sc_selfplay_report): what the searches of many slots found -- lines
ranked by visits, their principal variations, values and scores -- read from the trees on the GPU in one launch and one copy.

The ranking: visits descending, then the generator's order, so line 0 is the first most-visited child, the move mcts::step
(src/mcts.rs:309-311) and Play.step(temp=0) play.  A variation follows the most-visited child (ties: the lowest index) while the
node is expanded and that child has been visited.

Values: the search adds every evaluation up from White's point of view (search_select.hpp flips the sign for Black to move), so
`w` is White's; `q` = w / n is turned to the side to move at the root.  A terminal node carries no children but a header
(search_expand.hpp): -2 the game is drawn there (value 0: stalemate), -3 White has won (+1: Black is mated), -4 Black has won (-1);
the report's end codes for them are 1, 2 and 3, with 0 for a line that ends at an open node and 4 for one cut at 1024 moves."""
import ctypes as C
import math

import numpy as np

from .binding import MAX_MOVES, _check, _p, move_uci

END_OPEN, END_DRAW, END_WHITE_WON, END_BLACK_WON, END_DEPTH = range(5)
MAX_PV = 1024
# sc_report_slot
SLOT_DTYPE = np.dtype([(k, np.int32) for k in ("status", "ply", "sim", "n_nodes", "n_root_children", "root_children_n", "root_n", "turn",
                                               "n_lines", "pad")] + [("root_w", np.float32)])
LINE_ARRAYS = (("line_child", np.int32), ("line_n", np.int32), ("line_w", np.float32), ("line_prior", np.float32),
               ("line_len", np.int32), ("line_end", np.int32))


def line_q(w, n, turn):
    """the mean value of a child, float32, for the side to move at the root (turn 1: White); 0 without a visit"""
    if n == 0:
        return np.float32(0.0)
    q = np.float32(w) / np.float32(n)
    return q if turn == 1 else -q


def centipawns(q):
    """the formula of the reference's scripts/elo.py on the expected score s = (q + 1) / 2, clamped to [0.001, 0.999]"""
    s = min(max((float(q) + 1.0) / 2.0, 0.001), 0.999)
    return int(round(400.0 * math.log10(s / (1.0 - s))))


def line_score(q, length, end):
    """("mate", m) for a variation that ends in a decided game -- the mate is given by whoever made its last move: +(len + 1) // 2
    for an odd length (the side to move at the root), -(len // 2) for an even one -- else ("cp", centipawns(q))"""
    if end in (END_WHITE_WON, END_BLACK_WON):
        return ("mate", (length + 1) // 2 if length & 1 else -(length // 2))
    return ("cp", centipawns(q))


def report_arrays(n, multipv, pv_cap, fill=0):
    """the output arrays of one report: every byte `fill`"""
    out = {"info": np.zeros(max(n, 1), SLOT_DTYPE)[:n]}
    for k, dt in LINE_ARRAYS:
        out[k] = np.zeros((n, multipv), dt)
    out["pv"] = np.zeros((n, multipv, pv_cap), np.uint16)
    if fill:
        for a in out.values():
            a.view(np.uint8)[...] = fill
    return out


class Report(dict):
    """the arrays of one report: slots [n], the fields of sc_report_slot [n] each, line_child / line_n / line_w / line_prior /
    line_len / line_end [n][multipv], pv [n][multipv][pv_cap] (uint16 move words); rows from n_lines[i] on and moves behind
    min(line_len, pv_cap) are not written.  lines(i): the lines of entry i as dicts"""

    def lines(self, i):
        """-> [dict(move, pv (UCI strings: the first min(len, pv_cap) moves), child, n, w, q, prior, len, end, score)] by rank"""
        turn, cap = int(self["turn"][i]), self["pv"].shape[2]
        out = []
        for r in range(int(self["n_lines"][i])):
            n, w = int(self["line_n"][i, r]), self["line_w"][i, r]
            length, end = int(self["line_len"][i, r]), int(self["line_end"][i, r])
            pv = [move_uci(m) for m in self["pv"][i, r, :min(length, cap)]]
            q = line_q(w, n, turn)
            out.append(dict(move=pv[0] if pv else None, pv=pv, child=int(self["line_child"][i, r]), n=n, w=float(w), q=float(q),
                            prior=float(self["line_prior"][i, r]), len=length, end=end, score=line_score(q, length, end)))
        return out


def report(sp, slots=None, multipv=1, pv_cap=64, out=None):
    """sc_selfplay_report on a SelfPlay handle: slots (None: every slot of the handle), 1 <= multipv <= 224 lines per slot,
    0 <= pv_cap <= 1024 moves kept per variation -> Report.  out: arrays from report_arrays to write into"""
    if slots is None:
        n, sl = sp.cfg.n_slots, None
        listed = np.arange(n, dtype=np.int32)
    else:
        listed = sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        n = sl.size
    if not 1 <= multipv <= MAX_MOVES or not 0 <= pv_cap <= MAX_PV:
        raise ValueError("report: 1 <= multipv <= 224 and 0 <= pv_cap <= 1024")
    a = report_arrays(n, multipv, pv_cap) if out is None else out
    if a["pv"].shape != (n, multipv, pv_cap) or a["info"].shape != (n,):
        raise ValueError("report: `out` is not report_arrays(n, multipv, pv_cap)")
    _check(sp.L.sc_selfplay_report(sp.h, n, None if sl is None or n == 0 else _p(sl), multipv, pv_cap, _p(a["info"]),
                                   *[_p(a[k]) for k, _ in LINE_ARRAYS], _p(a["pv"])))
    rep = Report(slots=listed.copy(), pv=a["pv"])
    for k in SLOT_DTYPE.names:
        if k != "pad":
            rep[k] = a["info"][k]
    for k, _ in LINE_ARRAYS:
        rep[k] = a[k]
    return rep


def last_timing(L):
    """(kernel ms, whole-call ms) of this thread's last sc_selfplay_report"""
    k, t = C.c_float(0), C.c_float(0)
    L.sc_selfplay_report_last_timing(C.byref(k), C.byref(t))
    return k.value, t.value


def san_lines(rep, played=None, fens=None, device=0):
    """The variations of a report as SAN: -> per entry a list (by rank) of lists of SAN strings.  played: per entry the moves
    that lead from its base to the searched position (None: none), fens: per entry that base (a FEN string; None: the start
    position).  Rendered by the device's SAN writer (scamd.san.moves_to_san) in one call, the played moves in front of every
    variation and only the tail kept."""
    from .san import moves_to_san
    n = len(rep["n_lines"])
    played = [list(p or ()) for p in (played if played is not None else [None] * n)]
    fens = list(fens) if fens is not None else [None] * n
    if len(played) != n or len(fens) != n:
        raise ValueError("san_lines: one move list and one base per entry of the report")
    cap = rep["pv"].shape[2]
    games, gfens, owner = [], [], []
    for i in range(n):
        for r in range(int(rep["n_lines"][i])):
            games.append(played[i] + [int(m) for m in rep["pv"][i, r, :min(int(rep["line_len"][i, r]), cap)]])
            gfens.append(fens[i])
            owner.append(i)
    out = [[] for _ in range(n)]
    if not games:
        return out
    sans, status = moves_to_san(games, fens=gfens if any(f is not None for f in gfens) else None, device=device)
    for g, i in enumerate(owner):
        if status[g]:
            raise ValueError(f"san_lines: entry {i}: move {-int(status[g]) - 1} of a line is not legal from the given base and moves")
        out[i].append(sans[g][len(played[i]):])
    return out
