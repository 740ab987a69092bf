"""Positions given as FEN / EPD text (csrc/fen_text.cpp, csrc/fen_kernels.hip, csrc/positions.hip): the base of a move list for
the encoder, a search, a match line or a SAN game.  The text is read on the host; whether a position can be played is decided on
the GPU, where the rules are."""
import ctypes as C

import numpy as np

from .binding import MAX_MOVES, EngineError, _check, _count, _Handle, _p, lib

# sc_positions_status: what a negative code says (include/sc_engine.h)
STATUS_TEXT = {0: "playable", 1: "the game is over here", -1: "not exactly one king per side", -2: "a pawn on rank 1 or 8",
               -3: "the side that is not to move is in check", -4: "material no game can reach", -5: "more than two checkers",
               -6: "contradicting fields", -101: "bad board field", -102: "bad turn field", -103: "bad castling field",
               -104: "bad ep field", -105: "bad halfmove clock", -106: "bad fullmove number"}
FIELDS = ("board", "turn", "castling", "ep", "halfmove", "fullmove")   # sc_fen_parse returns -(1 + index) of the failing one


class FenFields(C.Structure):
    """sc_fen_fields"""
    _fields_ = [("pcs", C.c_uint64 * 6), ("occ", C.c_uint64 * 2), ("turn", C.c_int32), ("castling", C.c_int32), ("ep", C.c_int32),
                ("halfmove", C.c_int32), ("fullmove", C.c_int32), ("reserved", C.c_int32)]


def parse_fen(text):
    """sc_fen_parse (no GPU needed): FEN / EPD text -> FenFields with the raw fields; ValueError names the failing field"""
    raw = text.encode() if isinstance(text, str) else bytes(text)
    f = FenFields()
    rc = lib().sc_fen_parse(raw, len(raw), C.byref(f))
    if rc:
        raise ValueError(f"bad FEN ({FIELDS[-rc - 1]} field): {text!r}" if -6 <= rc <= -1 else f"sc_fen_parse: error {rc}")
    return f


class Positions(_Handle):
    """sc_positions: a set of positions in GPU memory, validated there.  fens: FEN / EPD strings, None for the start position.
    .status[i]: 0 playable, 1 the game is over, < 0 refused (STATUS_TEXT); .fen(i): python-chess's Board.fen() of entry i."""
    _destroy = "sc_positions_destroy"

    def __init__(self, fens, device=0):
        self.L = lib()
        self.device = device
        fens = list(fens)
        n = len(fens)
        arr = (C.c_char_p * max(n, 1))(*[None if f is None else (f.encode() if isinstance(f, str) else bytes(f)) for f in fens])
        status = np.zeros(max(n, 1), np.int32)
        self.h = h = C.c_void_p()
        _check(self.L.sc_positions_from_fen(device, n, arr, C.byref(h), _p(status)))
        self.status = status[:n].copy()

    def __len__(self):
        return int(self.L.sc_positions_count(self.h))

    def fen(self, i):
        buf = C.create_string_buffer(128)
        _count(self.L.sc_positions_fen(self.h, i, buf, 128))
        return buf.value.decode()

    def check(self, for_search=False):
        """raises EngineError for the first entry that cannot be used (negative status; with for_search also status 1)"""
        for i, st in enumerate(self.status):
            if st < 0 or (st == 1 and for_search):
                raise EngineError(f"position {i}: {STATUS_TEXT.get(int(st), int(st))}")
        return self


def bases_of(fens, n, device):
    """the `fens=` argument of the entry points that take bases -> (Positions or None, base_idx int32 [n] or None, owned): fens is
    None, a list of n FEN strings / None, or a Positions of n entries; owned: the caller closes the set after its call"""
    if fens is None:
        return None, None, False
    if isinstance(fens, Positions):
        if len(fens) != n:
            raise ValueError(f"{len(fens)} positions for {n} move lists")
        return fens, np.arange(n, dtype=np.int32), False
    fens = list(fens)
    if len(fens) != n:
        raise ValueError(f"{len(fens)} FENs for {n} move lists")
    if all(f is None for f in fens):
        return None, None, False
    idx = np.full(max(n, 1), -1, np.int32)
    texts = []
    for i, f in enumerate(fens):
        if f is not None:
            idx[i] = len(texts)
            texts.append(f)
    return Positions(texts, device), idx, True


def analyse(engine, fens, rollout, cpuct=2.5, best=None, evaluator="net", seed=0, device=0, trees=False, multipv=1, pv_cap=64):
    """A suite of positions in `rollout` launches: one position per slot of one handle (SelfPlay.set_position from a base for
    each), one enqueue of `rollout` simulations, then ONE report of every slot (SelfPlay.report): the root children, the move
    and the lines come from it.
    -> dict(results=[dict(fen, move, children=[(uci, N, Q, prior), ...], pv, score, lines) per position], solved=count or None).
    move: the first most-visited child; pv / score: its principal variation (UCI strings, pv_cap >= 1 of them at most) and
    ("cp", c) or ("mate", m); lines: the first `multipv` lines by visits as scamd.report.Report.lines gives them.  best: per
    position a UCI move or a collection of them (an EPD `bm`, once resolved through scamd.san); solved counts the positions whose
    move is among them.  trees: every result also carries the slot's whole tree (SelfPlay.tree)."""
    if not 1 <= multipv <= MAX_MOVES or not 1 <= pv_cap <= 1024:
        raise ValueError("analyse: 1 <= multipv <= 224 and 1 <= pv_cap <= 1024")
    from .selfplay import SelfPlay
    pos = fens if isinstance(fens, Positions) else Positions(fens, engine.device if engine is not None else device)
    owned = pos is not fens
    try:
        pos.check(for_search=True)
        n = len(pos)
        if best is not None and len(best) != n:
            raise ValueError(f"{len(best)} best moves for {n} positions")
        results, solved = [], (0 if best is not None else None)
        if n == 0:
            return dict(results=results, solved=solved)
        sp = SelfPlay(engine, n_slots=n, n_games=n, rollout_num=max(rollout + 1, 512), num_steps=4000, cpuct=cpuct, with_noise=False,
                      outcome_gate=1 << 30, evaluator=evaluator, seed=seed, device=device)
        try:
            for i in range(n):
                sp.set_position(i, [], fen=(pos, i))
            _check(sp.L.sc_selfplay_set_search(sp.h, cpuct, 0.15, 0))
            sp.enqueue(rollout)
            sp.sync()
            sp.check_flags("analyse")   # (a blocked position searched deeper than 1024 levels: no numbers from such a tree)
            rep = sp.report(multipv=MAX_MOVES, pv_cap=pv_cap)   # every root child of every slot is a line: one launch, one copy
            for i in range(n):
                lines = rep.lines(i)
                ch = [(ln["move"], ln["n"], ln["w"], ln["prior"]) for ln in sorted(lines, key=lambda ln: ln["child"])]
                r = dict(fen=pos.fen(i), move=lines[0]["move"] if lines else None, children=ch)
                if trees:
                    r["tree"] = sp.tree(i)
                r.update(pv=lines[0]["pv"] if lines else [], score=lines[0]["score"] if lines else None, lines=lines[:multipv])
                mv = r["move"]
                results.append(r)
                if best is not None:
                    want = {best[i]} if isinstance(best[i], str) else set(best[i])
                    solved += int(mv in want)
        finally:
            sp.close()
        return dict(results=results, solved=solved)
    finally:
        if owned:
            pos.close()

