"""The device rules asked directly (csrc/perft_kernels.hip, csrc/perft.hip): perft -- node counts, the divide, the kinds of the last
moves -- and the legal moves of positions, from the start position or from FEN bases.  Imports `binding` and `fen` only; its
names are not re-exported from `scamd`."""
import ctypes as C

import numpy as np

from .binding import MAX_MOVES, _check, _moves, _p, lib, move_uci
from .fen import bases_of

KINDS = ("captures", "ep", "castles", "promotions", "checks", "checkmates")   # SC_PERFT_CAPTURES .. SC_PERFT_CHECKMATES: slots 1..6


def perft(move_lists, depth, fens=None, device=0, divide=False, kinds=False, max_frontier=0):
    """sc_perft for entries given as move lists (uint16 moves or UCI strings), each from the start position or from its base
    (`fens` as encode_positions takes it: FEN strings, None for the start position, or a scamd.fen.Positions of as many entries).
    -> dict(nodes=uint64 [n], status=int32 [n] (0, or -(j+1): move j of the list is not legal)); with kinds also
    kinds=dict(captures=..., ep=..., castles=..., promotions=..., checks=..., checkmates=...) of uint64 [n] over the last moves;
    with divide also divide=[[(uci, count), ...] per entry] in the generator's order.  max_frontier (0: the library's 2^20)
    changes the memory the walk uses, never its results."""
    L = lib()
    ml = [list(g) for g in move_lists]
    n = len(ml)
    pos, bidx, owned = bases_of(fens, n, device)
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum([len(g) for g in ml])
    flat = _moves([m for g in ml for m in g])
    n1 = max(n, 1)
    nodes = np.zeros(n1, np.uint64)
    status = np.zeros(n1, np.int32)
    kd = np.zeros((n1, 8), np.uint64) if kinds else None
    dm = np.zeros((n1, MAX_MOVES), np.uint16) if divide else None
    dn = np.zeros((n1, MAX_MOVES), np.uint64) if divide else None
    nd = np.zeros(n1, np.int32) if divide else None
    try:
        _check(L.sc_perft(device, n, pos.h if pos is not None else None, _p(bidx), _p(flat), _p(off), int(depth), int(max_frontier),
                          _p(nodes), _p(kd), _p(dm), _p(dn), _p(nd), _p(status)))
    finally:
        if owned:
            pos.close()
    out = dict(nodes=nodes[:n], status=status[:n])
    if kinds:
        out["kinds"] = {name: kd[:n, 1 + k].copy() for k, name in enumerate(KINDS)}
    if divide:
        out["divide"] = [[(move_uci(dm[i, k]), int(dn[i, k])) for k in range(nd[i])] for i in range(n)]
    return out


def legal_moves(move_lists, fens=None, device=0):
    """the legal moves of every entry as UCI strings, in the generator's order (python-chess's): the divide at depth 1.  An entry
    whose move list is not legal raises ValueError."""
    r = perft(move_lists, 1, fens=fens, device=device, divide=True)
    bad = np.flatnonzero(r["status"])
    if bad.size:
        raise ValueError(f"entry {int(bad[0])}: move {-int(r['status'][bad[0]]) - 1} of its list is not legal")
    return [[u for u, _ in row] for row in r["divide"]]


def last_timing():
    """(kernel ms, whole-call ms) of this thread's last sc_perft"""
    a, b = C.c_float(0), C.c_float(0)
    lib().sc_perft_last_timing(C.byref(a), C.byref(b))
    return a.value, b.value
