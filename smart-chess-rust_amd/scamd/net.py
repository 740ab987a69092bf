"""The network handle and the rules + encoder entry point (csrc/engine.hip): Engine, encode_positions, ChessHip."""
import ctypes as C

import numpy as np

from .binding import MAX_MOVES, EngineError, NetConfig, _check, _Handle, _moves, _p, _stream, _torch, _tp, lib


def _planes(boards, meta):
    """-> boards int8 [n,8,8,112], meta int32 [n,7] as contiguous arrays, and n"""
    boards = np.ascontiguousarray(boards, np.int8).reshape(-1, 8, 8, 112)
    meta = np.ascontiguousarray(meta, np.int32).reshape(-1, 7)
    return boards, meta, boards.shape[0]


def _check_reference_tensors(torch, boards, meta, device):
    """boards / meta of layout="reference" (int8 [n,8,8,112], int32 [n,7]) on cuda:<device>; the trainer layout is refused
    -> the number of positions"""
    if boards.dtype != torch.int8 or meta.dtype != torch.int32 or tuple(boards.shape[1:]) != (8, 8, 112) or tuple(meta.shape[1:]) != (7,):
        raise ValueError('boards / meta are not in the reference layout (int8 [P,8,8,112], int32 [P,7]): encode them with '
                         'layout="reference" -- the network kernels read the planes as the encoder writes them, not the '
                         "trainer's float32 [P,112,8,8]")
    for name, t in (("boards", boards), ("meta", meta)):
        if not t.is_cuda or t.device.index != device or not t.is_contiguous():
            raise ValueError(f"{name}: a contiguous tensor on cuda:{device} is needed")
    if meta.shape[0] != boards.shape[0]:
        raise ValueError("boards and meta differ in their number of positions")
    return boards.shape[0]


class Engine(_Handle):
    """The network backend (replaces ChessTS/ChessEP/ChessOnnx construction, src/main.rs:83-128)."""
    _destroy = "sc_engine_destroy"

    def __init__(self, n_res_blocks=10, channels=256, seed=0, weights=None, device=0, precision="bf16"):
        self.L = lib()
        self.n_res_blocks, self.channels = n_res_blocks, channels
        self.device = device
        cfg = NetConfig(n_res_blocks, channels, seed, {"bf16": 0, "fp8": 1}[precision], 0)
        self.h = h = C.c_void_p()   # null until the library fills it in: close() leaves a null handle alone
        _check(self.L.sc_engine_create(C.byref(cfg), weights.encode() if weights else None, device, C.byref(h)))
        self.precision = "fp8" if self.L.sc_engine_precision(h) == 1 else "bf16"   # an SCW2 blob decides by itself

    def forward(self, boards, meta, want_logp=True):
        """ChessModule.forward: boards int8[n,8,8,112], meta int32[n,7] -> logp[n,4672], value[n]"""
        boards, meta, n = _planes(boards, meta)
        logp = np.zeros((n, 4672), np.float32) if want_logp else None
        value = np.zeros(n, np.float32)
        _check(self.L.sc_forward_batch(self.h, n, _p(boards), _p(meta), _p(logp), _p(value)))
        return logp, value

    def forward_torch(self, boards, meta, want_logp=True):
        """sc_forward_device: ChessModule.forward on torch tensors of this engine's GPU -- boards int8 [n,8,8,112], meta int32 [n,7]
        (layout="reference") -> (logp float32 [n,4672] or None, value float32 [n]), enqueued on torch.cuda.current_stream();
        bit-identical to forward()"""
        torch = _torch()
        n = _check_reference_tensors(torch, boards, meta, self.device)
        dev = torch.device("cuda", self.device)
        logp = torch.empty((n, 4672), dtype=torch.float32, device=dev) if want_logp else None
        value = torch.empty(n, dtype=torch.float32, device=dev)
        _check(self.L.sc_forward_device(self.h, n, _tp(boards), _tp(meta), _stream(torch, self.device), _tp(logp), _tp(value)))
        return logp, value

    def debug(self, boards, meta, stage):
        boards, meta, n = _planes(boards, meta)
        out = np.zeros((n, 64, self.channels), np.float32)
        _check(self.L.sc_forward_debug(self.h, n, _p(boards), _p(meta), stage, _p(out)))
        return out

    def predict(self, boards, meta, legal_idx, argmax=False):
        """Game::predict tail: legal_idx = list (per position) of action indices -> (list of priors, value[n]);
        argmax: post_process_distr's one-hot branch (src/chess.rs:880-889)"""
        boards, meta, n = _planes(boards, meta)
        off = np.zeros(n + 1, np.uint32)
        off[1:] = np.cumsum([len(x) for x in legal_idx])
        flat = np.ascontiguousarray(np.concatenate([np.asarray(x, np.uint16) for x in legal_idx]) if off[-1] else
                                    np.zeros(0, np.uint16), np.uint16)
        pri = np.zeros(int(off[-1]), np.float32)
        value = np.zeros(n, np.float32)
        fn = self.L.sc_predict_batch_argmax if argmax else self.L.sc_predict_batch
        _check(fn(self.h, n, _p(boards), _p(meta), _p(flat), _p(off), _p(pri), _p(value)))
        return [pri[off[i]:off[i + 1]] for i in range(n)], value


def encode_positions(move_lists, device=0, engine=None, fens=None):
    """Rules + encoder on the GPU for positions given as move lists (uint16 moves or UCI strings).
    fens: per move list the position it starts from (sc_encode_positions_from) -- FEN strings, None for the start position -- or
    a scamd.fen.Positions of as many entries; history planes older than a base are zero."""
    from .fen import bases_of
    L = lib()
    ml = [list(g) for g in move_lists]
    n = len(ml)
    dev = engine.device if engine is not None else device
    pos, bidx, owned = bases_of(fens, n, dev)
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum([len(g) for g in ml])
    flat = _moves([m for g in ml for m in g])
    boards = np.zeros((n, 8, 8, 112), np.int8)
    meta = np.zeros((n, 7), np.int32)
    lm = np.zeros((n, MAX_MOVES), np.uint16)
    li = np.zeros((n, MAX_MOVES), np.uint16)
    nl = np.zeros(n, np.int32)
    oc = np.zeros((n, 4), np.int32)
    try:
        if pos is None:
            _check(L.sc_encode_positions(engine.h if engine else None, device, n, _p(flat), _p(off), _p(boards), _p(meta), _p(lm),
                                         _p(li), _p(nl), _p(oc)))
        else:
            _check(L.sc_encode_positions_from(engine.h if engine else None, device, n, pos.h, _p(bidx), _p(flat), _p(off), _p(boards),
                                              _p(meta), _p(lm), _p(li), _p(nl), _p(oc)))
    finally:
        if owned:
            pos.close()
    return dict(boards=boards, meta=meta, legal_moves=[lm[i, :nl[i]].copy() for i in range(n)],
                legal_idx=[li[i, :nl[i]].copy() for i in range(n)], n_legal=nl, termination=oc[:, 0], winner=oc[:, 1],
                is_check=oc[:, 2], status=oc[:, 3])


class ChessHip:
    """Mirror of `impl Game<BoardState> for ChessTS` (src/backends/torch.rs:34-53) over the GPU engine.

    A node/state pair of the reference is represented by the list of moves played from the start
    position (that is what `_encode` reconstructs from the tree's parent chain and the board's
    move stack, src/chess.rs:845-867).
    """

    def __init__(self, engine):
        self.engine = engine

    def predict(self, moves, argmax=False, fen=None):
        """-> (steps, priors, value): steps = legal moves (uint16) in python-chess order; empty at game end,
        with value = +1 White won / -1 Black won / 0 (torch.rs:98-106).  fen: the position the moves start from"""
        enc = encode_positions([moves], engine=self.engine, fens=None if fen is None else [fen])
        if enc["status"][0] < 0:
            raise EngineError(f"illegal move at index {-enc['status'][0] - 1}")
        if enc["n_legal"][0] == 0:
            w = enc["winner"][0]
            return [], np.zeros(0, np.float32), (1.0 if w == 1 else -1.0 if w == 0 else 0.0)
        pri, val = self.engine.predict(enc["boards"], enc["meta"], [enc["legal_idx"][0]], argmax=argmax)
        return list(enc["legal_moves"][0]), pri[0], float(val[0])

    @staticmethod
    def reverse_q(moves):
        """node.step.1 == Black (torch.rs:49-52): Black is to move after an odd number of plies"""
        return len(moves) % 2 == 1
