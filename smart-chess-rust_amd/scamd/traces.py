"""Trace files read on the GPU (csrc/trace_kernels.hip, csrc/traces.hip): the text of many files goes up in one copy, kernels find
the played moves, the children with their visit counts, the outcome and the optional "opening" / "fen" members, and the encoder
reads the packed arrays where they are.  A reader of machine-written traces (sc_selfplay_write_trace_json, the reference's
Trace::save, json.dumps of the same shape), not a JSON validator: include/sc_engine.h has the contract."""
import ctypes as C

import numpy as np

from .binding import EngineError, _check, _count, _Handle, _moves, _p, _stream, _torch, lib, move_uci
from .training import _device_outputs, _finish_outputs

# SC_TRACE_ERR_* (include/sc_engine.h): status[g] = -code of a refused file
ERR_UNBALANCED, ERR_ESCAPE, ERR_STEPS, ERR_SHAPE, ERR_MOVE, ERR_COUNT, ERR_CHILDREN, ERR_PLIES, ERR_OUTCOME, ERR_SPACE = range(1, 11)
ERR_NAMES = {1: "UNBALANCED", 2: "ESCAPE", 3: "STEPS", 4: "SHAPE", 5: "MOVE", 6: "COUNT", 7: "CHILDREN", 8: "PLIES", 9: "OUTCOME", 10: "SPACE"}
# csrc/trace_json.hpp TERMINATION_NAMES
TERMINATION_NAMES = ("", "Checkmate", "Stalemate", "InsufficientMaterial", "SeventyfiveMoves", "FivefoldRepetition", "FiftyMoves",
                     "ThreefoldRepetition", "VariantWin", "VariantLoss", "VariantDraw")
STATUS_REFUSED, STATUS_HAS_BASE = 300000, 400000   # sc_traces_encode_device: + code; the file has "opening" or "fen"
MAX_PLIES, MAX_TEXT = 4000, (1 << 32) - 1


class Traces(_Handle):
    """sc_traces: n parsed trace files in GPU memory.  Per file (numpy): status (0, or -ERR_*), err_at (byte offset of the first
    defect), n_steps, n_children, n_opening, has_outcome, termination, winner (sc_trace_info's conventions: 1 White, 0 Black,
    -1 none), has_fen, and outcomes -- White's result, float32: 1 / -1 / 0, 0 also without an outcome."""
    _destroy = "sc_traces_destroy"

    def __init__(self, text, text_off, device=0):
        self.L = lib()
        self.device = device
        text_off = np.ascontiguousarray(text_off, np.uint64)
        n = text_off.size - 1
        self.h = h = C.c_void_p()
        _check(self.L.sc_traces_read(device, n, text, _p(text_off), C.byref(h)))
        self.n = n
        m = max(n, 1)
        self.status, self.has_fen, oc = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros((m, 3), np.int32)
        self.err_at, self.n_steps, self.n_children, self.n_opening = (np.zeros(m, np.uint32) for _ in range(4))
        _check(self.L.sc_traces_summary(h, _p(self.status), _p(self.err_at), _p(self.n_steps), _p(self.n_children), _p(self.n_opening),
                                        _p(oc), _p(self.has_fen)))
        for k in ("status", "has_fen", "err_at", "n_steps", "n_children", "n_opening"):
            setattr(self, k, getattr(self, k)[:n])
        self.has_outcome, self.termination, self.winner = (oc[:n, k].copy() for k in range(3))
        self.outcomes = np.where(self.has_outcome == 1, np.where(self.winner == 1, 1.0, np.where(self.winner == 0, -1.0, 0.0)), 0.0).astype(np.float32)

    def __len__(self):
        return self.n

    def _range(self, g0, n):
        n = self.n - g0 if n is None else n
        if g0 < 0 or n < 0 or g0 + n > self.n:
            raise ValueError(f"games [{g0}, {g0 + n}) of {self.n}")
        return g0, n

    def moves(self, g0=0, n=None):
        """-> (moves uint16 [P], move_off uint32 [n + 1]) of games [g0, g0 + n), offsets rebased to 0 (sc_traces_get)"""
        g0, n = self._range(g0, n)
        off = np.zeros(n + 1, np.uint32)
        _check(self.L.sc_traces_get(self.h, g0, n, _p(off), None, None, None, None, None, None))
        mv = np.zeros(max(int(off[n]), 1), np.uint16)
        _check(self.L.sc_traces_get(self.h, g0, n, None, _p(mv), None, None, None, None, None))
        return mv[:int(off[n])], off

    def children(self, g0=0, n=None):
        """-> (child_mv uint16 [C], child_n uint32 [C], child_off uint32 [P + 1]) of games [g0, g0 + n), offsets rebased to 0"""
        g0, n = self._range(g0, n)
        P, Cn = int(self.n_steps[g0:g0 + n].sum()), int(self.n_children[g0:g0 + n].sum())
        coff, cm, cn = np.zeros(P + 1, np.uint32), np.zeros(max(Cn, 1), np.uint16), np.zeros(max(Cn, 1), np.uint32)
        _check(self.L.sc_traces_get(self.h, g0, n, None, None, _p(coff), _p(cm), _p(cn), None, None))
        return cm[:Cn], cn[:Cn], coff

    def openings(self):
        """-> per file the list of its "opening" moves as UCI strings ([] without the member)"""
        off, op = np.zeros(self.n + 1, np.uint32), np.zeros(max(int(self.n_opening.sum()), 1), np.uint16)
        _check(self.L.sc_traces_get(self.h, 0, self.n, None, None, None, None, None, _p(off), _p(op)))
        return [[move_uci(m) for m in op[off[g]:off[g + 1]]] for g in range(self.n)]

    def fens(self):
        """-> per file its "fen" member, or None"""
        out, buf = [], C.create_string_buffer(128)
        for g in range(self.n):
            k = _count(self.L.sc_traces_fen(self.h, g, buf, 128)) if self.has_fen[g] else 0
            out.append(buf.value.decode() if k else None)
        return out

    def games(self, g0=0, n=None):
        """-> the list form encode_steps_batch takes, [[(move, [(move, count), ...]), ...] per game] with UCI strings"""
        g0, n = self._range(g0, n)
        mv, off = self.moves(g0, n)
        cm, cn, coff = self.children(g0, n)
        return [[(move_uci(mv[p]), [(move_uci(cm[c]), int(cn[c])) for c in range(coff[p], coff[p + 1])]) for p in range(off[g], off[g + 1])]
                for g in range(n)]

    def check(self, names=None):
        """raises EngineError naming every refused file with its code name and the offset of the defect"""
        bad = np.nonzero(self.status < 0)[0]
        if bad.size:
            raise EngineError("refused trace files: " + "; ".join(
                f"{names[g] if names is not None else g}: {ERR_NAMES.get(-int(self.status[g]), int(self.status[g]))} at byte {int(self.err_at[g])}"
                for g in bad))
        return self


def read(sources, device=0):
    """sc_traces_read: sources are paths (read with open(..., "rb")), bytes objects, or a mix -> Traces"""
    lib()
    blobs = []
    for s in sources:
        if isinstance(s, (bytes, bytearray, memoryview)):
            blobs.append(bytes(s))
        else:
            with open(s, "rb") as f:
                blobs.append(f.read())
    off = np.zeros(len(blobs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in blobs], dtype=np.uint64)
    return Traces(b"".join(blobs), off, device)


def pack_traces(traces):
    """trace dicts in SelfPlay.trace's shape (steps [(uci, q, [(uci, N, Q, uct), ...]), ...], outcome; optional "opening": list of
    moves, "fen": str) -> the argument list of sc_traces_format behind its device and count, up to `fens` (numpy arrays are kept
    alive by the list)"""
    from .binding import TERMINATION, TraceInfo
    term = {v: k for k, v in TERMINATION.items()}
    n = len(traces)
    info = (TraceInfo * max(n, 1))()
    steps = [s for t in traces for s in t["steps"]]
    ch = [c for s in steps for c in s[2]]
    step_off, open_off = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32)
    for g, t in enumerate(traces):
        oc = t.get("outcome")
        info[g].n_steps = len(t["steps"])
        info[g].n_children_total = sum(len(s[2]) for s in t["steps"])
        info[g].has_outcome = int(oc is not None)
        info[g].termination = term[oc["termination"]] if oc else 0
        info[g].winner = {"White": 1, "Black": 0, None: -1}[oc["winner"]] if oc else -1
        info[g].game_id = int(t.get("game_id", 0))
        step_off[g + 1] = step_off[g] + len(t["steps"])
        open_off[g + 1] = open_off[g] + len(t.get("opening") or ())
    child_off = np.zeros(len(steps) + 1, np.uint32)
    child_off[1:] = np.cumsum([len(s[2]) for s in steps], dtype=np.uint64)
    sm, sq = _moves([s[0] for s in steps]), np.asarray([s[1] for s in steps] or [0], np.float32)
    cm, cn = _moves([c[0] for c in ch]), np.asarray([c[1] for c in ch] or [0], np.int32)
    cq, cu = np.asarray([c[2] for c in ch] or [0], np.float32), np.asarray([c[3] for c in ch] or [0], np.float32)
    op = _moves([m for t in traces for m in (t.get("opening") or ())])
    fens = (C.c_char_p * max(n, 1))(*[t["fen"].encode() if t.get("fen") else None for t in traces])
    return [info, _p(step_off), _p(sm), _p(sq), _p(child_off), _p(cm), _p(cn), _p(cq), _p(cu), _p(open_off), _p(op), fens], \
        (step_off, sm, sq, child_off, cm, cn, cq, cu, open_off, op)


def format(traces, device=0):
    """sc_traces_format: the trace-file text of every trace dict, formatted on the GPU in one call -> list of bytes, each exactly
    what write_trace_json writes for it (a trace may also carry "opening" and "fen", written behind "steps")"""
    L = lib()
    n = len(traces)
    args, keep = pack_traces(traces)
    off = np.zeros(n + 1, np.uint64)
    _check(L.sc_traces_format(device, n, *args, None, 0, _p(off)))
    text = np.zeros(max(int(off[n]), 1), np.uint8)
    _check(L.sc_traces_format(device, n, *args, _p(text), int(off[n]), _p(off)))
    del keep
    return [text[int(off[g]):int(off[g + 1])].tobytes() for g in range(n)]


def write(paths, traces, device=0):
    """format(traces), trace g written to paths[g]"""
    paths = list(paths)
    if len(paths) != len(traces):
        raise ValueError("one path per trace")
    for p, t in zip(paths, format(traces, device)):
        with open(p, "wb") as f:
            f.write(t)


def format_last_timing():
    """(count_ms, emit_ms) of this thread's last device format call (sc_traces_format_last_timing)"""
    a, b = C.c_float(0), C.c_float(0)
    lib().sc_traces_format_last_timing(C.byref(a), C.byref(b))
    return a.value, b.value


def encode_traces_torch(traces, g0=0, n=None, apply_mirror=False, layout="trainer", dist="dense", engine=None):
    """Games [g0, g0 + n) of a Traces -> the dict of encode_steps_torch (sc_traces_encode_device): the moves and children never
    leave the GPU.  outcome comes from the parsed outcomes.  status: 0, 1000 + i / -(i + 1) as encode_steps_torch,
    STATUS_REFUSED + code for a refused file (no plies), STATUS_HAS_BASE for a file with "opening" or "fen"."""
    torch = _torch()
    g0, n = traces._range(g0, n)
    dev = traces.device
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum(traces.n_steps[g0:g0 + n], dtype=np.uint64)
    out, args = _device_outputs(torch, dev, int(off[n]), n, layout, dist)
    _check(traces.L.sc_traces_encode_device(engine.h if engine else None, traces.h, g0, n, int(bool(apply_mirror)), args[0],
                                            _stream(torch, dev), *args[1:]))
    return _finish_outputs(torch, out, off, traces.outcomes[g0:g0 + n], apply_mirror, dev)


def batches(paths, max_bytes=1 << 30, device=0):
    """A long list of files in calls of at most max_bytes of text each (a call takes less than 4 GiB): yields (Traces,
    paths_of_the_batch); a single file above max_bytes gets a batch of its own.  The caller closes each Traces."""
    import os
    max_bytes = min(int(max_bytes), MAX_TEXT)
    group, size = [], 0
    for p in paths:
        k = os.path.getsize(p)
        if group and size + k > max_bytes:
            yield read(group, device), group
            group, size = [], 0
        group.append(p)
        size += k
    if group:
        yield read(group, device), group
