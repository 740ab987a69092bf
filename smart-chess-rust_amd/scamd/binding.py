"""ctypes binding of include/sc_engine.h (libsc_engine.so)."""
import ctypes as C
import os

# see INTEGRATION.md: kernel arguments in device memory (must precede HIP runtime initialisation)
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SC_ENGINE_LIB: developer override (experiment builds of the same library); there is still no CPU fallback
_LIB_PATH = os.environ.get("SC_ENGINE_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libsc_engine.so")

MAX_MOVES = 224
TERMINATION = {0: None, 1: "Checkmate", 2: "Stalemate", 3: "InsufficientMaterial", 4: "SeventyfiveMoves",
               5: "FivefoldRepetition", 6: "FiftyMoves", 7: "ThreefoldRepetition"}
_WINNER = {1: "White", 0: "Black", -1: None}
EVALUATORS = {"net": 0, "synth": 1, "synth_coarse": 2, "synth_uniform": 3}   # SC_EVAL_* (include/sc_engine.h)


class EngineError(RuntimeError):
    code = None


ERR_HANDOFF = -5   # SC_ERR_HANDOFF: the self-play handle is poisoned (include/sc_engine.h)


class NetConfig(C.Structure):
    _fields_ = [("n_res_blocks", C.c_int32), ("channels", C.c_int32), ("seed", C.c_uint64), ("precision", C.c_int32),
                ("reserved", C.c_int32)]


class SelfplayConfig(C.Structure):
    _fields_ = [("n_slots", C.c_int32), ("n_games", C.c_int32), ("rollout_num", C.c_int32), ("num_steps", C.c_int32),
                ("cpuct", C.c_float), ("temperature", C.c_float), ("temperature_switch", C.c_int32),
                ("epsilon", C.c_float), ("with_noise", C.c_int32), ("outcome_gate", C.c_int32),
                ("evaluator", C.c_int32), ("external_noise", C.c_int32), ("seed", C.c_uint64),
                ("first_game_id", C.c_uint64), ("trace_capacity", C.c_int32), ("own_stream", C.c_int32),
                ("tie_random", C.c_int32), ("trace_hold", C.c_int32), ("rollout_factor", C.c_float)]


class Stats(C.Structure):
    _fields_ = [("sims_done", C.c_int64), ("nn_evals", C.c_int64), ("games_finished", C.c_int32),
                ("games_active", C.c_int32), ("error_flags", C.c_int32), ("plies_done", C.c_int32)]


class TraceInfo(C.Structure):
    _fields_ = [("n_steps", C.c_int32), ("n_children_total", C.c_int32), ("has_outcome", C.c_int32),
                ("termination", C.c_int32), ("winner", C.c_int32), ("game_id", C.c_uint64)]


# every symbol include/sc_engine.h declares: name -> (restype, argtypes)
_vp, _i, _i64, _u16p, _f = C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_float
ABI = {
    "sc_last_error": (C.c_char_p, []),
    "sc_device_count": (_i, []),
    "sc_runtime_flags": (_i, []),
    "sc_last_warning": (C.c_char_p, []),
    "sc_selfplay_poll": (_i, [_vp, _vp, _i]),
    "sc_debug_find_max": (_i, [_i, _vp, _i, _vp]),
    "sc_debug_choose_child": (_i, [_i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "sc_selfplay_debug_break_handoff": (_i, [_vp, _i]),
    "sc_debug_clear_handoff_failure": (_i, [_i]),
    "sc_selfplay_debug_cycles": (_i, [_vp, _i, _vp]),
    "sc_engine_create": (_i, [C.POINTER(NetConfig), C.c_char_p, _i, C.POINTER(_vp)]),
    "sc_engine_destroy": (None, [_vp]),
    "sc_engine_max_batch": (_i, [_vp]),
    "sc_engine_precision": (_i, [_vp]),
    "sc_forward_batch": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "sc_predict_batch": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_predict_batch_argmax": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_engine_synchronize": (_i, [_vp]),
    "sc_forward_debug": (_i, [_vp, _i, _vp, _vp, _i, _vp]),
    "sc_encode_positions": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_selfplay_create": (_i, [_vp, _i, C.POINTER(SelfplayConfig), C.POINTER(_vp)]),
    "sc_selfplay_destroy": (None, [_vp]),
    "sc_selfplay_enqueue_sims": (_i, [_vp, _i]),
    "sc_selfplay_synchronize": (_i, [_vp]),
    "sc_selfplay_enqueue_interleaved": (_i, [_vp, _i, _i]),
    "sc_selfplay_run": (_i, [_vp, _i64]),
    "sc_selfplay_get_stats": (_i, [_vp, C.POINTER(Stats)]),
    "sc_search": (_i, [_vp, _vp, _i, _i, _f, _i, C.c_uint64, _i, _vp, _vp, _vp, _vp, _vp]),
    "sc_selfplay_set_search": (_i, [_vp, _f, _f, _i]),
    "sc_selfplay_set_players": (_i, [_vp, _vp, _vp, C.c_uint64, C.c_uint64]),
    "sc_selfplay_enable_timing": (_i, [_vp, _i]),
    "sc_selfplay_timing": (_i, [_vp, _i, C.POINTER(_f), C.POINTER(_f), C.POINTER(_i64)]),
    "sc_selfplay_launches_per_step": (_i, [_vp]),
    "sc_selfplay_get_trace": (_i, [_vp, _i, C.POINTER(TraceInfo), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_selfplay_write_trace_json": (_i, [_vp, _i, C.c_char_p]),
    "sc_selfplay_get_tree": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_selfplay_get_slot": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_selfplay_set_noise": (_i, [_vp, _i, _vp, _i]),
    "sc_selfplay_get_noise": (_i, [_vp, _i, _vp, _i]),
    "sc_selfplay_set_position": (_i, [_vp, _i, _vp, _i]),
    "sc_encode_steps_last_timing": (_i, [C.POINTER(_f), C.POINTER(_f)]),
    "sc_encode_steps": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_encode_steps_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_selfplay_encode_traces": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_forward_device": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "sc_score_positions": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_compare_engines": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_gather_batch": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_trace_write_json": (_i, [C.c_char_p, C.POINTER(TraceInfo), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_move_uci": (_i, [C.c_uint16, C.c_char_p]),
    "sc_move_index": (_i, [C.c_uint16, _i]),
}

_lib = None
_engine_hip = []   # libamdhip64 file(s) libsc_engine.so bound to when it was loaded


def lib_path():
    return _LIB_PATH


def lib():
    """Loads libsc_engine.so; raises EngineError (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise EngineError(f"{_LIB_PATH} is missing: build it with `python smart-chess-rust_amd/build.py` "
                          "(there is no CPU fallback)")
    before = set(hip_runtime_files())
    try:
        L = C.CDLL(_LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise EngineError(f"cannot load {_LIB_PATH}: {e}") from e
    # the HIP runtime the engine bound to: the one its loading mapped, or the one already there (a host that loaded torch first)
    global _engine_hip
    new = set(hip_runtime_files()) - before
    _engine_hip = sorted(new or before)
    for name, (res, args) in ABI.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        e = EngineError(f"libsc_engine error {rc}: {lib().sc_last_error().decode()}")
        e.code = rc
        raise e


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def move_uci(m):
    buf = C.create_string_buffer(8)
    lib().sc_move_uci(int(m), buf)
    return buf.value.decode()


def uci_move(s):
    promo = {"n": 2, "b": 3, "r": 4, "q": 5}
    f = (ord(s[1]) - 49) * 8 + ord(s[0]) - 97
    t = (ord(s[3]) - 49) * 8 + ord(s[2]) - 97
    return f | (t << 6) | ((promo[s[4]] if len(s) > 4 else 0) << 12)


class Engine:
    """The network backend (replaces ChessTS/ChessEP/ChessOnnx construction, src/main.rs:83-128)."""

    def __init__(self, n_res_blocks=10, channels=256, seed=0, weights=None, device=0, precision="bf16"):
        self.L = lib()
        self.n_res_blocks, self.channels = n_res_blocks, channels
        self.device = device
        cfg = NetConfig(n_res_blocks, channels, seed, {"bf16": 0, "fp8": 1}[precision], 0)
        h = C.c_void_p()
        _check(self.L.sc_engine_create(C.byref(cfg), weights.encode() if weights else None, device, C.byref(h)))
        self.h = h
        self.precision = "fp8" if self.L.sc_engine_precision(h) == 1 else "bf16"   # an SCW2 blob decides by itself

    def close(self):
        if getattr(self, "h", None):
            self.L.sc_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def forward(self, boards, meta, want_logp=True):
        """ChessModule.forward: boards int8[n,8,8,112], meta int32[n,7] -> logp[n,4672], value[n]"""
        boards = np.ascontiguousarray(boards, np.int8).reshape(-1, 8, 8, 112)
        meta = np.ascontiguousarray(meta, np.int32).reshape(-1, 7)
        n = boards.shape[0]
        logp = np.zeros((n, 4672), np.float32) if want_logp else None
        value = np.zeros(n, np.float32)
        _check(self.L.sc_forward_batch(self.h, n, _p(boards), _p(meta), _p(logp), _p(value)))
        return logp, value

    def forward_torch(self, boards, meta, want_logp=True):
        """sc_forward_device: ChessModule.forward on torch tensors of this engine's GPU -- boards int8 [n,8,8,112], meta int32 [n,7]
        (layout="reference") -> (logp float32 [n,4672] or None, value float32 [n]), enqueued on torch.cuda.current_stream();
        bit-identical to forward()"""
        torch = _torch_for_device()
        _check_reference_tensors(torch, boards, meta, self.device)
        n = boards.shape[0]
        dev = torch.device("cuda", self.device)
        logp = torch.empty((n, 4672), dtype=torch.float32, device=dev) if want_logp else None
        value = torch.empty(n, dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(self.device)
        _check(self.L.sc_forward_device(self.h, n, _tp(boards), _tp(meta), C.c_void_p(stream.cuda_stream), _tp(logp), _tp(value)))
        return logp, value

    def debug(self, boards, meta, stage):
        boards = np.ascontiguousarray(boards, np.int8).reshape(-1, 8, 8, 112)
        meta = np.ascontiguousarray(meta, np.int32).reshape(-1, 7)
        n = boards.shape[0]
        out = np.zeros((n, 64, self.channels), np.float32)
        _check(self.L.sc_forward_debug(self.h, n, _p(boards), _p(meta), stage, _p(out)))
        return out

    def predict(self, boards, meta, legal_idx, argmax=False):
        """Game::predict tail: legal_idx = list (per position) of action indices -> (list of priors, value[n]);
        argmax: post_process_distr's one-hot branch (src/chess.rs:880-889)"""
        boards = np.ascontiguousarray(boards, np.int8).reshape(-1, 8, 8, 112)
        meta = np.ascontiguousarray(meta, np.int32).reshape(-1, 7)
        n = boards.shape[0]
        off = np.zeros(n + 1, np.uint32)
        off[1:] = np.cumsum([len(x) for x in legal_idx])
        flat = np.ascontiguousarray(np.concatenate([np.asarray(x, np.uint16) for x in legal_idx]) if off[-1] else
                                    np.zeros(0, np.uint16), np.uint16)
        pri = np.zeros(int(off[-1]), np.float32)
        value = np.zeros(n, np.float32)
        fn = self.L.sc_predict_batch_argmax if argmax else self.L.sc_predict_batch
        _check(fn(self.h, n, _p(boards), _p(meta), _p(flat), _p(off), _p(pri), _p(value)))
        return [pri[off[i]:off[i + 1]] for i in range(n)], value


def encode_positions(move_lists, device=0, engine=None):
    """Rules + encoder on the GPU for positions given as move lists (uint16 moves or UCI strings)."""
    L = lib()
    n = len(move_lists)
    ml = [[uci_move(m) if isinstance(m, str) else int(m) for m in g] for g in move_lists]
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum([len(g) for g in ml])
    flat = np.asarray([m for g in ml for m in g], np.uint16)
    if flat.size == 0:
        flat = np.zeros(1, np.uint16)
    boards = np.zeros((n, 8, 8, 112), np.int8)
    meta = np.zeros((n, 7), np.int32)
    lm = np.zeros((n, MAX_MOVES), np.uint16)
    li = np.zeros((n, MAX_MOVES), np.uint16)
    nl = np.zeros(n, np.int32)
    oc = np.zeros((n, 4), np.int32)
    _check(L.sc_encode_positions(engine.h if engine else None, device, n, _p(flat), _p(off), _p(boards), _p(meta), _p(lm),
                                 _p(li), _p(nl), _p(oc)))
    return dict(boards=boards, meta=meta, legal_moves=[lm[i, :nl[i]].copy() for i in range(n)],
                legal_idx=[li[i, :nl[i]].copy() for i in range(n)], n_legal=nl, termination=oc[:, 0], winner=oc[:, 1],
                is_check=oc[:, 2], status=oc[:, 3])


def encode_steps_batch(games, apply_mirror=False, device=0, engine=None):
    """Trace -> training tensors for a batch of games on the GPU (sc_encode_steps).
    games: list of step lists [(next_move, [(move, count), ...]), ...] with moves as uint16 or UCI strings -- the
    `steps` argument of libsmartchess.chess_encode_steps (reference src/lib.rs:46-50), one per game.
    -> dict(boards int8[P,8,8,112], meta int32[P,7], dist f32[P,4672], move_indices [P lists], ply_off[n+1], status[n])"""
    L = lib()
    flat, off, cm, cn, coff = pack_steps(games)
    n, P = len(games), int(off[-1])
    boards = np.zeros((max(P, 1), 8, 8, 112), np.int8)
    meta = np.zeros((max(P, 1), 7), np.int32)
    dist = np.zeros((max(P, 1), 4672), np.float32)
    li = np.zeros((max(P, 1), MAX_MOVES), np.uint16)
    nl = np.zeros(max(P, 1), np.int32)
    status = np.zeros(max(n, 1), np.int32)
    _check(L.sc_encode_steps(engine.h if engine else None, device, n, _p(flat), _p(off), _p(cm), _p(cn), _p(coff),
                             int(bool(apply_mirror)), _p(boards), _p(meta), _p(dist), _p(li), _p(nl), _p(status)))
    return dict(boards=boards[:P], meta=meta[:P], dist=dist[:P], move_indices=[li[i, :nl[i]].astype(np.int32) for i in range(P)],
                ply_off=off, status=status[:n])


def pack_steps(games):
    """The list form of encode_steps_batch -> the packed arrays (moves, move_off, child_mv, child_n, child_off) that
    sc_encode_steps / sc_encode_steps_device take"""
    mv = lambda m: uci_move(m) if isinstance(m, str) else int(m)
    n = len(games)
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum([len(g) for g in games])
    P = int(off[n])
    flat = np.asarray([mv(s[0]) for g in games for s in g] or [0], np.uint16)
    coff = np.zeros(P + 1, np.uint32)
    coff[1:] = np.cumsum([len(s[1]) for g in games for s in g])
    cm = np.asarray([mv(c[0]) for g in games for s in g for c in s[1]] or [0], np.uint16)
    cn = np.asarray([int(c[1]) for g in games for s in g for c in s[1]] or [0], np.uint32)
    return flat, off, cm, cn, coff


def hip_runtime_files():
    """the distinct libamdhip64 files mapped into this process (/proc/self/maps)"""
    found = set()
    with open("/proc/self/maps") as f:
        for ln in f:
            parts = ln.split(None, 5)
            if len(parts) == 6 and os.path.basename(parts[5].strip()).startswith("libamdhip64"):
                found.add(os.path.realpath(parts[5].strip()))
    return sorted(found)


def hip_runtime():
    """ctypes handle of the HIP runtime libsc_engine.so uses (device buffers for the *_device entry points without torch)"""
    lib()
    if len(_engine_hip) != 1:
        raise EngineError(f"cannot tell which HIP runtime libsc_engine.so uses: {_engine_hip}")
    return C.CDLL(_engine_hip[0])


_LAYOUTS = {"reference": 0, "trainer": 1}
_DISTS = ("dense", "legal", "both")


def _torch_for_device():
    """torch, after checking that it shares the engine's HIP runtime: device pointers must not cross between two runtimes"""
    L = lib()
    if L.sc_device_count() <= 0:
        raise EngineError("no HIP device available: libsc_engine has no CPU fallback")
    import torch
    files = hip_runtime_files()
    if len(files) > 1:
        raise EngineError(f"two HIP runtimes are loaded ({', '.join(files)}): torch was imported after scamd loaded "
                          "libsc_engine.so -- import torch before scamd")
    return torch


def _device_outputs(torch, device, P, n, layout, dist):
    if layout not in _LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(_LAYOUTS)}")
    if dist not in _DISTS:
        raise ValueError(f"dist must be one of {_DISTS}")
    lay = _LAYOUTS[layout]
    dev = torch.device("cuda", device)
    R = max(P, 1)
    out = {}
    if lay == 1:
        out["boards"] = torch.empty((R, 112, 8, 8), dtype=torch.float32, device=dev)
        out["meta"] = torch.empty((R, 7), dtype=torch.float32, device=dev)
    else:
        out["boards"] = torch.empty((R, 8, 8, 112), dtype=torch.int8, device=dev)
        out["meta"] = torch.empty((R, 7), dtype=torch.int32, device=dev)
    out["dist"] = torch.empty((R, 4672), dtype=torch.float32, device=dev) if dist in ("dense", "both") else None
    out["dist_legal"] = torch.empty((R, MAX_MOVES), dtype=torch.float32, device=dev) if dist in ("legal", "both") else None
    out["legal_idx"] = torch.empty((R, MAX_MOVES), dtype=torch.int16, device=dev)   # action indices < 4672: exact in int16
    out["n_legal"] = torch.empty(R, dtype=torch.int32, device=dev)
    out["status"] = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    args = [lay] + [ptr(out[k]) for k in ("boards", "meta", "dist", "dist_legal", "legal_idx", "n_legal", "status")]
    return out, args


def _finish_outputs(torch, out, ply_off, outcome_per_game, apply_mirror, device):
    n = ply_off.size - 1
    P = int(ply_off[n])
    status = out.pop("status")[:n].cpu().numpy()   # the one host copy: waits for the work on the current stream
    res = {k: (None if v is None else v[:P]) for k, v in out.items()}
    oc = np.repeat(np.asarray(outcome_per_game, np.float32), np.diff(ply_off.astype(np.int64)))
    if apply_mirror:
        oc = -oc   # ChessDataset negates the outcome under the mirror (py/dataset.py)
    res["outcome"] = torch.from_numpy(oc).to(torch.device("cuda", device))
    res["ply_off"] = ply_off
    res["status"] = status
    return res


def encode_steps_torch(games, apply_mirror=False, layout="trainer", dist="dense", engine=None, device=0, outcomes=None):
    """Training tensors on the GPU, for a trainer there (sc_encode_steps_device): no copy through the host.
    games: the list form of encode_steps_batch, or the packed arrays (moves, move_off, child_mv, child_n, child_off) as a
    tuple or a dict with those keys (pack_steps).  layout "trainer": boards float32 [P,112,8,8] and meta float32 [P,7]
    (py/dataset.py _prepare); "reference": int8 [P,8,8,112] and int32 [P,7] as encode_steps_batch.  dist "dense": dist
    float32 [P,4672]; "legal": dist_legal float32 [P,224] aligned with legal_idx (rebuild the dense rows with
    zeros(P, 4672).scatter_add_(1, legal_idx.long(), dist_legal) -- scatter_add_, not scatter_: padding entries point at action
    0); "both".  outcomes: per game, White's result (1, -1, 0; None: 0) -> outcome float32 [P], negated under apply_mirror as
    ChessDataset does.
    -> dict of torch tensors on cuda:<device> (enqueued on torch.cuda.current_stream()): boards, meta, dist, dist_legal,
    legal_idx (int16) [P,224], n_legal int32 [P], outcome; plus ply_off (numpy) and status (numpy, sc_encode_steps's codes)."""
    L = lib()
    if L.sc_device_count() <= 0:
        raise EngineError("no HIP device available: libsc_engine has no CPU fallback")
    if isinstance(games, dict):
        packed = tuple(games[k] for k in ("moves", "move_off", "child_mv", "child_n", "child_off"))
    elif isinstance(games, tuple) and len(games) == 5 and all(isinstance(a, np.ndarray) for a in games):
        packed = games
    else:
        packed = pack_steps(games)
    flat, off, cm, cn, coff = (np.ascontiguousarray(a, t) for a, t in zip(packed, (np.uint16, np.uint32, np.uint16, np.uint32, np.uint32)))
    n = off.size - 1
    torch = _torch_for_device()
    dev = engine.device if engine is not None else device
    out, args = _device_outputs(torch, dev, int(off[n]), n, layout, dist)
    stream = torch.cuda.current_stream(dev)
    _check(L.sc_encode_steps_device(engine.h if engine else None, dev, n, _p(flat if flat.size else np.zeros(1, np.uint16)), _p(off),
                                    _p(cm if cm.size else np.zeros(1, np.uint16)), _p(cn if cn.size else np.zeros(1, np.uint32)),
                                    _p(coff), int(bool(apply_mirror)), args[0], C.c_void_p(stream.cuda_stream), *args[1:]))
    oc = np.zeros(n, np.float32) if outcomes is None else np.asarray(outcomes, np.float32)
    return _finish_outputs(torch, out, off, oc, apply_mirror, dev)


def _tp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _check_reference_tensors(torch, boards, meta, device):
    """boards / meta of layout="reference" (int8 [n,8,8,112], int32 [n,7]) on cuda:<device>; the trainer layout is refused"""
    if boards.dtype != torch.int8 or meta.dtype != torch.int32 or tuple(boards.shape[1:]) != (8, 8, 112) or tuple(meta.shape[1:]) != (7,):
        raise ValueError('boards / meta are not in the reference layout (int8 [P,8,8,112], int32 [P,7]): encode them with '
                         'layout="reference" -- the network kernels read the planes as the encoder writes them, not the '
                         "trainer's float32 [P,112,8,8]")
    for name, t in (("boards", boards), ("meta", meta)):
        if not t.is_cuda or t.device.index != device or not t.is_contiguous():
            raise ValueError(f"{name}: a contiguous tensor on cuda:{device} is needed")
    if meta.shape[0] != boards.shape[0]:
        raise ValueError("boards and meta differ in their number of positions")


SCORE_SUMMARY = ("n", "loss1", "loss2", "pi_entropy", "n_nonfinite")
COMPARE_SUMMARY = ("n", "tv_mean", "tv_std", "tv_max", "tv_min", "dv_mean", "dv_std", "dv_max", "dv_min")


def score_torch(engine, tensors):
    """A network judged on recorded search results (sc_score_positions; the reference's validation_step and pi_entropy).
    tensors: the dict encode_steps_torch(..., layout="reference") / SelfPlay.training_tensors(..., layout="reference")
    returns -- boards, meta, outcome and the visit shares as dist (dense) or dist_legal + legal_idx + n_legal (with
    dist="both" the sparse form is used: 21 x fewer bytes).
    -> dict: per-position torch tensors ce, se, ent, value (float32 [P], on the GPU), floats loss1 = mean ce, loss2 = mean se,
    pi_entropy = mean ent, ints n and n_nonfinite (positions whose ce, se or ent is not finite; they stay in the means).
    Enqueued on torch.cuda.current_stream(); the summary's copy to the host waits for it."""
    torch = _torch_for_device()
    boards, meta = tensors["boards"], tensors["meta"]
    _check_reference_tensors(torch, boards, meta, engine.device)
    n = boards.shape[0]
    dist, dl, li, nl = (tensors.get(k) for k in ("dist", "dist_legal", "legal_idx", "n_legal"))
    if dl is not None and li is not None and nl is not None:
        dist = None
        if dl.dtype != torch.float32 or li.dtype not in (torch.int16, getattr(torch, "uint16", torch.int16)) or nl.dtype != torch.int32:
            raise ValueError("dist_legal float32, legal_idx int16 and n_legal int32 are needed")
        sparse = (dl, li, nl)
    elif dist is not None:
        if dist.dtype != torch.float32:
            raise ValueError("dist: float32 is needed")
        sparse = (None, None, None)
    else:
        raise ValueError("the visit shares are missing: dist, or dist_legal + legal_idx + n_legal")
    outcome = tensors["outcome"]
    dev = torch.device("cuda", engine.device)
    for name, t, rows in (("dist", dist, n), ("dist_legal", sparse[0], n), ("legal_idx", sparse[1], n), ("n_legal", sparse[2], n),
                          ("outcome", outcome, n)):
        if t is not None and (t.device != dev or not t.is_contiguous() or t.shape[0] != rows):
            raise ValueError(f"{name}: a contiguous tensor of {rows} rows on cuda:{engine.device} is needed")
    if outcome.dtype != torch.float32:
        raise ValueError("outcome: float32 is needed")
    out = {k: torch.empty(n, dtype=torch.float32, device=dev) for k in ("ce", "se", "ent", "value")}
    summary = torch.empty(len(SCORE_SUMMARY), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(engine.device)
    _check(engine.L.sc_score_positions(engine.h, n, _tp(boards), _tp(meta), _tp(dist), _tp(sparse[0]), _tp(sparse[1]), _tp(sparse[2]),
                                       _tp(outcome), C.c_void_p(stream.cuda_stream), _tp(out["ce"]), _tp(out["se"]), _tp(out["ent"]),
                                       _tp(out["value"]), _tp(summary)))
    s = summary.cpu().tolist()
    out.update(n=int(s[0]), loss1=s[1], loss2=s[2], pi_entropy=s[3], n_nonfinite=int(s[4]))
    return out


def compare_torch(engine_a, engine_b, tensors):
    """Agreement of two networks on the same positions (sc_compare_engines; the reference's scripts/validate_model.py).
    tensors: a dict with boards and meta in layout="reference" on the engines' GPU.
    -> dict: per-position torch tensors tv (total variation of the two policies) and dv (|value_a - value_b|), and the floats
    tv_mean, tv_std, tv_max, tv_min, dv_mean, dv_std, dv_max, dv_min (population standard deviation), int n."""
    torch = _torch_for_device()
    boards, meta = tensors["boards"], tensors["meta"]
    _check_reference_tensors(torch, boards, meta, engine_a.device)
    n = boards.shape[0]
    dev = torch.device("cuda", engine_a.device)
    out = {k: torch.empty(n, dtype=torch.float32, device=dev) for k in ("tv", "dv")}
    summary = torch.empty(len(COMPARE_SUMMARY), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(engine_a.device)
    _check(engine_a.L.sc_compare_engines(engine_a.h, engine_b.h, n, _tp(boards), _tp(meta), C.c_void_p(stream.cuda_stream),
                                         _tp(out["tv"]), _tp(out["dv"]), _tp(summary)))
    s = summary.cpu().tolist()
    out.update({k: v for k, v in zip(COMPARE_SUMMARY[1:], s[1:])}, n=int(s[0]))
    return out


_torch_checked = None


def _torch_once():
    """_torch_for_device() on the first call, its result afterwards: the per-batch calls do not read /proc/self/maps again"""
    global _torch_checked
    if _torch_checked is None:
        _torch_checked = _torch_for_device()
    return _torch_checked


def _check_compact_tensors(torch, src):
    """the compact training tensors (layout="reference" with the sparse visit shares) on one GPU -> (device index, rows)"""
    boards, meta = src.get("boards"), src.get("meta")
    if boards is None or meta is None:
        raise ValueError("boards / meta are missing")
    if not boards.is_cuda:
        raise ValueError("boards: a tensor on the GPU is needed")
    device = boards.device.index
    _check_reference_tensors(torch, boards, meta, device)
    n = boards.shape[0]
    dl, li, nl, oc = (src.get(k) for k in ("dist_legal", "legal_idx", "n_legal", "outcome"))
    if dl is None or li is None or nl is None:
        raise ValueError('the sparse visit shares (dist_legal + legal_idx + n_legal) are missing: encode with dist="legal" or '
                         'dist="both" -- dense rows are gathered with torch.index_select')
    if oc is None:
        raise ValueError("outcome is missing")
    if dl.dtype != torch.float32 or li.dtype not in (torch.int16, getattr(torch, "uint16", torch.int16)) or nl.dtype != torch.int32 \
            or oc.dtype != torch.float32:
        raise ValueError("dist_legal float32, legal_idx int16, n_legal int32 and outcome float32 are needed")
    dev = torch.device("cuda", device)
    for name, t, shape in (("dist_legal", dl, (n, MAX_MOVES)), ("legal_idx", li, (n, MAX_MOVES)), ("n_legal", nl, (n,)), ("outcome", oc, (n,))):
        if t.device != dev or not t.is_contiguous() or tuple(t.shape) != shape:
            raise ValueError(f"{name}: a contiguous tensor of shape {shape} on cuda:{device} is needed")
    return device, n


def gather_batch_torch(src, rows, mirror=None, n_bad=None):
    """A trainer-layout minibatch from rows of the compact tensors (sc_gather_batch; the reference's DataLoader over ChessDataset
    and _prepare, py/dataset.py:31-87), without leaving the GPU and without a dense dist in memory.
    src: the dict encode_steps_torch(..., layout="reference", dist="legal" | "both") / SelfPlay.training_tensors(...) returns (or
    any dict of boards, meta, dist_legal, legal_idx, n_legal, outcome in that form); rows: int32 / int64 cuda tensor [B] of row
    numbers (a row may repeat); mirror: None, or a cuda tensor [B] (bool / uint8) -- non-zero: the colour-mirrored sample (meta
    of Board::rotate(), outcome negated); n_bad: None, or an int32 cuda tensor [1] that receives the number of samples with bad
    input (row outside the source: all NaN; n_legal outside 0..218 or an action index >= 4672: dist NaN).
    -> (boards float32 [B,112,8,8], meta float32 [B,7], dist float32 [B,4672], outcome float32 [B,1]), enqueued on
    torch.cuda.current_stream()."""
    torch = _torch_once()
    device, n = _check_compact_tensors(torch, src)
    dev = torch.device("cuda", device)
    if rows.dtype not in (torch.int32, torch.int64) or rows.dim() != 1 or rows.device != dev:
        raise ValueError(f"rows: a one-dimensional int32 or int64 tensor on cuda:{device} is needed")
    rows = rows.to(torch.int32).contiguous()
    B = rows.shape[0]
    if mirror is not None:
        if mirror.device != dev or tuple(mirror.shape) != (B,):
            raise ValueError(f"mirror: a tensor of shape ({B},) on cuda:{device} is needed")
        if mirror.dtype == torch.bool:
            mirror = mirror.view(torch.uint8)
        elif mirror.dtype != torch.uint8:
            mirror = (mirror != 0).to(torch.uint8)
        mirror = mirror.contiguous()
    if n_bad is not None and (n_bad.device != dev or n_bad.dtype != torch.int32 or n_bad.numel() < 1):
        raise ValueError(f"n_bad: an int32 tensor on cuda:{device} is needed")
    out = (torch.empty((B, 112, 8, 8), dtype=torch.float32, device=dev), torch.empty((B, 7), dtype=torch.float32, device=dev),
           torch.empty((B, 4672), dtype=torch.float32, device=dev), torch.empty((B, 1), dtype=torch.float32, device=dev))
    stream = torch.cuda.current_stream(device)
    _check(lib().sc_gather_batch(device, n, B, _tp(rows), _tp(mirror), _tp(src["boards"]), _tp(src["meta"]), _tp(src["dist_legal"]),
                                 _tp(src["legal_idx"]), _tp(src["n_legal"]), _tp(src["outcome"]), C.c_void_p(stream.cuda_stream),
                                 _tp(out[0]), _tp(out[1]), _tp(out[2]), _tp(out[3]), _tp(n_bad)))
    return out


PLY_BYTES = 7168 + 28 + 4 * MAX_MOVES + 2 * MAX_MOVES + 4 + 4   # one ply of the compact tensors: 8 548


class ReplayIndex:
    """The bookkeeping of ReplayBuffer, in numpy (no GPU): whole games in a ring of `capacity` rows -- where a new game's plies
    go, which old games leave, which rows a trainer may draw (the reference's start_step rule) and how an epoch is cut."""

    def __init__(self, capacity, start_step=0):
        if capacity <= 0 or start_step < 0:
            raise ValueError("capacity must be positive and start_step non-negative")
        self.capacity, self.start_step = int(capacity), int(start_step)
        self.games = []     # oldest first: (first row, plies); a game's plies are consecutive rows modulo capacity
        self.head = 0       # the next row to be written
        self.used = 0
        self.version = 0    # changes with every add: a running epoch notices that its rows may be gone

    def add_games(self, lengths, status=None):
        """appends the games of one encode result (lengths[g] plies, starting at row sum(lengths[:g]) of it); games with a
        non-zero status or without plies are skipped; the oldest whole games leave until each new one fits.
        -> the copies to make, in order: [(source row, ring row, rows)], none of them wrapping"""
        lengths = [int(x) for x in lengths]
        status = [0] * len(lengths) if status is None else [int(x) for x in status]
        if len(status) != len(lengths):
            raise ValueError("one status per game is needed")
        for n, st in zip(lengths, status):
            if st == 0 and n > self.capacity:
                raise ValueError(f"a game of {n} plies does not fit a buffer of {self.capacity}")
        copies, src = [], 0
        for n, st in zip(lengths, status):
            if st == 0 and n > 0:
                while self.capacity - self.used < n:
                    self.used -= self.games.pop(0)[1]
                self.games.append((self.head, n))
                first = min(n, self.capacity - self.head)
                copies.append((src, self.head, first))
                if first < n:
                    copies.append((src + first, 0, n - first))
                self.head = (self.head + n) % self.capacity
                self.used += n
            src += n
        self.version += 1
        return copies

    def eligible_rows(self):
        """ring rows a trainer may draw, oldest game first: ChessDataset's rule (py/dataset.py:78-80), literally -- a game
        shorter than start_step keeps all its plies, any other its plies start_step: (one of exactly start_step plies: none)"""
        out = []
        for first, n in self.games:
            skip = 0 if n < self.start_step else self.start_step
            out.append((first + np.arange(skip, n, dtype=np.int64)) % self.capacity)
        return np.concatenate(out) if out else np.zeros(0, np.int64)

    @staticmethod
    def epoch_plan(n_eligible, batch_size, drop_last=True):
        """the batches of one epoch as slices [(lo, hi)] of the epoch's order"""
        if batch_size <= 0:
            raise ValueError("batch_size must be positive")
        n_full = n_eligible // batch_size
        plan = [(i * batch_size, (i + 1) * batch_size) for i in range(n_full)]
        if not drop_last and n_eligible % batch_size:
            plan.append((n_full * batch_size, n_eligible))
        return plan

    @staticmethod
    def epoch_seed(seed, epoch):
        """one 63-bit generator seed per (seed, epoch): splitmix64's finaliser over both"""
        z = (int(seed) * 0x9E3779B97F4A7C15 + int(epoch) + 1) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        return (z ^ (z >> 31)) & 0x7FFFFFFFFFFFFFFF


_COMPACT_KEYS = ("boards", "meta", "dist_legal", "legal_idx", "n_legal", "outcome")


class ReplayBuffer:
    """The reference's DataLoader(ConcatDataset([ChessDataset ...]), batch_size, shuffle=True, drop_last=True) over games kept
    on the GPU in the compact form (8 548 B per ply; allocated once, capacity_plies rows): add() appends the games of an encode
    result and evicts the oldest whole games, batches() yields shuffled trainer-layout minibatches built by sc_gather_batch."""

    def __init__(self, capacity_plies, device=0, start_step=0):
        self.index = ReplayIndex(capacity_plies, start_step)
        self.device = device
        self.store = None

    def __len__(self):
        return int(self.index.eligible_rows().size)

    def _storage(self):
        torch = _torch_once()
        if self.store is None:
            dev, n = torch.device("cuda", self.device), self.index.capacity
            self.store = dict(boards=torch.zeros((n, 8, 8, 112), dtype=torch.int8, device=dev),
                              meta=torch.zeros((n, 7), dtype=torch.int32, device=dev),
                              dist_legal=torch.zeros((n, MAX_MOVES), dtype=torch.float32, device=dev),
                              legal_idx=torch.zeros((n, MAX_MOVES), dtype=torch.int16, device=dev),
                              n_legal=torch.zeros(n, dtype=torch.int32, device=dev),
                              outcome=torch.zeros(n, dtype=torch.float32, device=dev))
            assert sum(t.element_size() * t[0].numel() for t in self.store.values()) == PLY_BYTES
        return torch

    def add(self, tensors):
        """the games of one encode_steps_torch(..., layout="reference", dist="legal" | "both") / SelfPlay.training_tensors
        result (games with status != 0 are skipped).  ValueError for a game longer than the buffer, before anything changes."""
        torch = self._storage()
        device, n = _check_compact_tensors(torch, tensors)
        if device != self.device:
            raise ValueError(f"the tensors are on cuda:{device}, the buffer on cuda:{self.device}")
        ply_off = np.asarray(tensors["ply_off"], np.int64)
        if int(ply_off[-1]) != n:
            raise ValueError("ply_off does not match the number of rows")
        for s, d, k in self.index.add_games(np.diff(ply_off), tensors["status"]):
            for key in _COMPACT_KEYS:
                self.store[key][d:d + k].copy_(tensors[key][s:s + k])

    def epoch_order(self, seed=0, epoch=0, shuffle=True, mirror=False):
        """the rows of one epoch in the order batches() draws them, and their mirror bits: (int32 [E], uint8 [E] or None) on the
        GPU.  The order is torch.randperm on the device from a generator seeded by (seed, epoch); mirror "random" takes one bit
        per sample from the same generator."""
        if mirror not in (False, True, "random"):
            raise ValueError('mirror must be False, True or "random"')
        torch = self._storage()
        dev = torch.device("cuda", self.device)
        order = torch.from_numpy(self.index.eligible_rows()).to(dev)
        E = order.shape[0]
        gen = torch.Generator(device=dev)
        gen.manual_seed(ReplayIndex.epoch_seed(seed, epoch))
        if shuffle:
            order = order[torch.randperm(E, generator=gen, device=dev)]
        if mirror == "random":
            bits = torch.randint(0, 2, (E,), generator=gen, device=dev, dtype=torch.uint8)
        else:
            bits = torch.ones(E, dtype=torch.uint8, device=dev) if mirror else None
        return order.to(torch.int32), bits

    def batches(self, batch_size, seed=0, epoch=0, shuffle=True, drop_last=True, mirror=False):
        """one epoch: yields (boards [B,112,8,8], meta [B,7], dist [B,4672], outcome [B,1]), float32 on the GPU, in the order of
        epoch_order(); mirror False / True / "random".  Nothing is copied to the host per batch.  An add() during the epoch ends
        it with a RuntimeError: the rows of the plan may have been evicted."""
        order, bits = self.epoch_order(seed, epoch, shuffle, mirror)
        plan = ReplayIndex.epoch_plan(int(order.shape[0]), batch_size, drop_last)
        return self._epoch(plan, order, bits)

    def _epoch(self, plan, order, bits):
        version = self.index.version
        for lo, hi in plan:
            if self.index.version != version:
                raise RuntimeError("games were added during the epoch: start a new one")
            yield gather_batch_torch(self.store, order[lo:hi], None if bits is None else bits[lo:hi])


def encode_steps_last_timing():
    """(kernel ms, whole-call ms) of this thread's last sc_encode_steps"""
    a, b = C.c_float(0), C.c_float(0)
    lib().sc_encode_steps_last_timing(C.byref(a), C.byref(b))
    return a.value, b.value


def encode_steps(steps, apply_mirror=False, device=0, engine=None):
    """Mirror of libsmartchess.chess_encode_steps(steps, apply_mirror) (reference src/lib.rs:46-128, used by
    py/dataset.py:77): one game -> [(boards int8[8,8,112], meta int32[7], dist f32[4672], move_indices), ...].
    Raises EngineError where the reference panics (children != legal moves, or an illegal played move)."""
    r = encode_steps_batch([steps], apply_mirror, device, engine)
    st = int(r["status"][0])
    if st >= 1000:
        raise EngineError(f"inconsistent moves at ply {st - 1000}")
    if st < 0:
        raise EngineError(f"num_act table doesn't include the next move (ply {-st - 1})")
    return [(r["boards"][i], r["meta"][i], r["dist"][i], r["move_indices"][i]) for i in range(len(steps))]


class Play:
    """Interactive engine handle: the `chess_play_*` functions of the reference's Python extension
    (src/lib.rs:161-358: new / mcts / step / apply_move / inspect / dump_search_tree / inference / encode) on one
    search slot of the GPU engine.  Differences: moves are UCI strings; `inspect()` returns the move list instead of a
    python-chess board object; the tree keeps only the current subtree (the reference also keeps the never revisited
    siblings of played moves), so `dump_search_tree()` shows the played line as a chain of single children."""

    def __init__(self, engine, initial_moves=(), evaluator="net", seed=0):
        self.engine = engine
        self.moves = [m if isinstance(m, str) else move_uci(m) for m in initial_moves]
        self._seed = seed
        # rollout_num is the per-ply budget of the self-play driver: huge here, plies advance only through step()
        self.sp = SelfPlay(engine, n_slots=1, n_games=1, rollout_num=60000, num_steps=4000, with_noise=False, outcome_gate=1 << 30,
                           evaluator=evaluator, seed=seed)
        self._rng = np.random.default_rng(seed)
        self._set()

    def _set(self):
        mv = np.asarray([uci_move(m) for m in self.moves] or [0], np.uint16)
        _check(self.sp.L.sc_selfplay_set_position(self.sp.h, 0, _p(mv), len(self.moves)))

    def close(self):
        self.sp.close()

    def mcts(self, rollout, cpuct=2.5, noise=False):
        """chess_play_mcts: `rollout` more simulations on the current tree (epsilon 0.15 as lib.rs:243)"""
        _check(self.sp.L.sc_selfplay_set_search(self.sp.h, cpuct, 0.15, int(bool(noise))))
        self.sp.enqueue(rollout)
        self.sp.sync()

    def _root_children(self):
        t = self.sp.tree(0)
        if t["n"].size == 0 or t["n_child"][0] == 0:
            return t, 0, 0
        return t, int(t["first_child"][0]), int(t["n_child"][0])

    def step(self, temp=0.0):
        """chess_play_step = mcts::step (src/mcts.rs:292-328): temperature 0 -> first most-visited child, else a
        sample ~ N^(1/temp); descends and starts a fresh tree there.  Returns the move or None (no children)."""
        t, fc, nc = self._root_children()
        if nc == 0:
            return None
        n = t["n"][fc:fc + nc].astype(np.float32)
        if temp == 0.0:
            choice = int(np.argmax(n))
        else:
            w = n ** np.float32(1.0 / temp)
            choice = int(self._rng.choice(nc, p=(w / w.sum()).astype(np.float64)))
        mv = move_uci(t["move"][fc + choice])
        self.apply_move(mv)
        return mv

    def apply_move(self, mov):
        """chess_play_apply_move: play `mov` and continue from a fresh node"""
        self.moves.append(mov if isinstance(mov, str) else move_uci(mov))
        self._set()

    def inspect(self):
        """chess_play_inspect -> (None, move stack newest first, q_value of the current node, [(move, N, Q), ...])"""
        t, fc, nc = self._root_children()
        q = float(t["q"][0]) if t["q"].size else 0.0
        ch = [(move_uci(t["move"][fc + i]), int(t["n"][fc + i]), float(t["q"][fc + i])) for i in range(nc)]
        return None, list(reversed(self.moves)), q, ch

    def dump_search_tree(self):
        """chess_play_dump_search_tree: nested dicts with serde's field names (src/mcts.rs:43-56: step, depth, q,
        num_act, children); step = [uci or None, colour of the side to move at the node]"""
        t = self.sp.tree(0)
        d0 = len(self.moves)

        def node(i, depth, mv):
            colour = "White" if depth % 2 == 0 else "Black"
            fc, nc = int(t["first_child"][i]), int(t["n_child"][i])
            kids = [node(fc + k, depth + 1, move_uci(t["move"][fc + k])) for k in range(nc)] if fc >= 0 else []
            return {"step": [mv, colour], "depth": depth, "q": float(t["q"][i]), "num_act": int(t["n"][i]), "children": kids}
        cur = node(0, d0, self.moves[-1] if self.moves else None) if t["n"].size else None
        for d in range(d0 - 1, -1, -1):   # the played line above the current node
            cur = {"step": [self.moves[d - 1] if d > 0 else None, "White" if d % 2 == 0 else "Black"], "depth": d, "q": 0.0,
                   "num_act": 0, "children": [cur]}
        return cur

    def inference(self):
        """chess_play_inference -> (legal moves, priors, value) of the current position (Game::predict)"""
        steps, pri, val = ChessHip(self.engine).predict(self.moves)
        return [move_uci(m) for m in steps], pri, val

    def encode(self):
        """chess_play_encode -> (boards int8[8,8,112], meta int32[7])"""
        e = encode_positions([self.moves], engine=self.engine)
        return e["boards"][0], e["meta"][0]


def encode_move(turn_white, move):
    """libsmartchess.chess_encode_move(turn, move) (reference src/lib.rs:37-44); no GPU needed"""
    return int(lib().sc_move_index(uci_move(move) if isinstance(move, str) else int(move), int(bool(turn_white))))


def search(engine, moves, rollout, cpuct=2.5, noise=False, seed=0):
    """sc_search: one search from the position after `moves` -> (root_q, [(uci, N, Q, prior), ...])"""
    mv = np.asarray([uci_move(m) if isinstance(m, str) else int(m) for m in moves] or [0], np.uint16)
    cm, cn = np.zeros(MAX_MOVES, np.uint16), np.zeros(MAX_MOVES, np.int32)
    cq, cp = np.zeros(MAX_MOVES, np.float32), np.zeros(MAX_MOVES, np.float32)
    rq = C.c_float(0)
    n = lib().sc_search(engine.h, _p(mv), len(moves), rollout, cpuct, int(bool(noise)), seed, MAX_MOVES, _p(cm), _p(cn), _p(cq), _p(cp),
                        C.byref(rq))
    if n < 0:
        _check(n)
    return rq.value, [(move_uci(cm[i]), int(cn[i]), float(cq[i]), float(cp[i])) for i in range(n)]


def elo(total, wins, losses):
    """scripts/elo.py:15-21: Elo difference from Total/Win/Lost"""
    import math
    s = (wins + (total - wins - losses) / 2) / total
    if s <= 0.0 or s >= 1.0:
        return math.copysign(math.inf, s - 0.5)
    return 400 * math.log(s / (1 - s), 10)


def play_match(a, b, n_games=100, rollout=100, cpuct=1.5, temperature=0.0, temperature_switch=0, num_steps=200, seed=0,
               swap=True):
    """Batched `scripts/leader-board:44-54`: n_games with engine `a` as White and `b` as Black, then (swap) the same
    number with the colours exchanged; every game is `play`'s loop (src/play.rs:241-343: no noise, outcome after every
    ply, at most 200 plies, random tie-break).  -> dict(results per colour assignment, a's score, Elo of a over b)."""
    out = {"as_white": None, "as_black": None}
    tot = win = lost = 0
    # Both colour assignments play at the same time: each handle launches on the stream of its White engine, so the two sets of
    # n_games workgroups share the GPU (100 + 100 of 256 CUs for the reference's 100-game matches) instead of running one after the
    # other.  A game depends only on its seed and id: the results are those of the sequential loop.
    handles = []
    for key, (w, bl) in (("as_white", (a, b)), ("as_black", (b, a))):
        if key == "as_black" and not swap:
            break
        sp = SelfPlay(w, n_slots=n_games, n_games=n_games, rollout_num=rollout, num_steps=num_steps, cpuct=cpuct,
                      temperature=temperature, temperature_switch=temperature_switch, with_noise=False, outcome_gate=-1,
                      seed=seed + (0 if key == "as_white" else 1), tie_random=True)
        sp.set_players(w, bl)
        handles.append((key, sp))
    live = [sp for _, sp in handles]
    while live:
        for _ in range(2):                       # two plies per look at the statistics
            if len(live) > 1:
                enqueue_interleaved(live, rollout)
            else:
                live[0].enqueue(rollout)
        live = [sp for sp in live if sp.stats()["games_active"] > 0]
    for key, sp in handles:
        res = {"White": 0, "Black": 0, "draw": 0, "unfinished": 0}
        traces = []
        for g in range(n_games):
            t = sp.trace(g)
            traces.append(t)
            oc = t["outcome"] if t else None
            if oc is None:
                res["unfinished"] += 1
            elif oc["winner"] is None:
                res["draw"] += 1
            else:
                res[oc["winner"]] += 1
        sp.close()
        out[key] = dict(results=res, traces=traces)
        a_col, b_col = ("White", "Black") if key == "as_white" else ("Black", "White")
        tot += n_games
        win += res[a_col]
        lost += res[b_col]
    out.update(total=tot, a_wins=win, b_wins=lost, elo_a_minus_b=elo(tot, win, lost))
    return out


class ChessHip:
    """Mirror of `impl Game<BoardState> for ChessTS` (src/backends/torch.rs:34-53) over the GPU engine.

    A node/state pair of the reference is represented by the list of moves played from the start
    position (that is what `_encode` reconstructs from the tree's parent chain and the board's
    move stack, src/chess.rs:845-867).
    """

    def __init__(self, engine):
        self.engine = engine

    def predict(self, moves, argmax=False):
        """-> (steps, priors, value): steps = legal moves (uint16) in python-chess order; empty at game end,
        with value = +1 White won / -1 Black won / 0 (torch.rs:98-106)."""
        enc = encode_positions([moves], engine=self.engine)
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


class SelfPlay:
    """Batched `selfplay` (src/main.rs): same option names as the reference CLI (main.rs:25-60)."""

    def __init__(self, engine=None, n_slots=256, n_games=None, rollout_num=180, num_steps=150, cpuct=2.5,
                 temperature=0.0, temperature_switch=4, epsilon=0.15, with_noise=True, outcome_gate=100,
                 evaluator="net", external_noise=False, seed=0, first_game_id=0, trace_capacity=0, own_stream=False, device=0,
                 tie_random=False, trace_hold=False, rollout_factor=0.0):
        self.L = lib()
        self.engine = engine
        self.device = engine.device if engine is not None else device
        cfg = SelfplayConfig(n_slots, n_games if n_games is not None else n_slots, rollout_num, num_steps, cpuct,
                             temperature, temperature_switch, epsilon, int(with_noise), outcome_gate,
                             EVALUATORS[evaluator], int(external_noise), seed, first_game_id, trace_capacity, int(own_stream),
                             int(tie_random), int(trace_hold), float(rollout_factor))
        self.cfg = cfg
        h = C.c_void_p()
        _check(self.L.sc_selfplay_create(engine.h if engine else None, device, C.byref(cfg), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.sc_selfplay_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def enqueue(self, n_sims):
        _check(self.L.sc_selfplay_enqueue_sims(self.h, n_sims))

    def set_players(self, white=None, black=None, salt_white=0, salt_black=0):
        """match play (src/play.rs:318-343): even plies are searched by `white`, odd plies by `black`"""
        self._players = (white, black)   # keep the engines alive
        _check(self.L.sc_selfplay_set_players(self.h, white.h if white else None, black.h if black else None, salt_white, salt_black))

    def sync(self):
        _check(self.L.sc_selfplay_synchronize(self.h))

    def run(self, max_sim_steps=0):
        _check(self.L.sc_selfplay_run(self.h, max_sim_steps))

    def stats(self):
        s = Stats()
        _check(self.L.sc_selfplay_get_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in Stats._fields_}

    def enable_timing(self, stride=1):
        _check(self.L.sc_selfplay_enable_timing(self.h, stride))

    def launches_per_step(self):
        """1: fused step kernel with the value FC inside, 2: fused step kernel + value FC launch, 3: separate launches"""
        return int(self.L.sc_selfplay_launches_per_step(self.h))

    def timing(self, reset=True):
        a, b, n = C.c_float(0), C.c_float(0), C.c_int64(0)
        _check(self.L.sc_selfplay_timing(self.h, int(reset), C.byref(a), C.byref(b), C.byref(n)))
        return dict(ms_total=a.value, ms_tower_sum=b.value, tower_launches=n.value)

    def poll(self, cap=4096):
        """sc_selfplay_poll: handle-local indices of the games that finished since they were last reported"""
        buf = np.zeros(max(cap, 1), np.int32)
        n = self.L.sc_selfplay_poll(self.h, _p(buf), cap)
        if n < 0:
            _check(n)
        return [int(x) for x in buf[:n]]

    def trace(self, game):
        """-> dict in the reference's trace-file shape (src/trace.rs:5-9); None if unfinished; raises EngineError when the
        trace has left the device (ring row overwritten or released)"""
        info = TraceInfo()
        rc = self.L.sc_selfplay_get_trace(self.h, game, C.byref(info), None, None, None, None, None, None, None)
        if rc == 1:
            return None
        _check(rc)
        ns, nc = info.n_steps, info.n_children_total
        sm, sq = np.zeros(ns + 1, np.uint16), np.zeros(ns + 1, np.float32)
        co = np.zeros(ns + 2, np.int32)
        cm, cn = np.zeros(nc + 1, np.uint16), np.zeros(nc + 1, np.int32)
        cq, cu = np.zeros(nc + 1, np.float32), np.zeros(nc + 1, np.float32)
        _check(self.L.sc_selfplay_get_trace(self.h, game, C.byref(info), _p(sm), _p(sq), _p(co), _p(cm), _p(cn), _p(cq),
                                            _p(cu)))
        steps = []
        for i in range(ns):
            ch = [(move_uci(cm[j]), int(cn[j]), float(cq[j]), float(cu[j])) for j in range(co[i], co[i + 1])]
            steps.append((move_uci(sm[i]), float(sq[i]), ch))
        outcome = None
        if info.has_outcome:
            outcome = {"termination": TERMINATION[info.termination], "winner": _WINNER[info.winner]}
        return {"steps": steps, "outcome": outcome, "game_id": int(info.game_id)}

    def training_tensors(self, games, apply_mirror=False, layout="trainer", dist="dense"):
        """Training tensors of finished games straight from the trace ring (sc_selfplay_encode_traces), as torch tensors on
        this handle's GPU -- see encode_steps_torch for the result.  outcome comes from the ring headers.  Raises EngineError
        with .code 1 if a game has not finished, 2 if its ring row has been overwritten or released."""
        games = np.ascontiguousarray(games, np.int32).reshape(-1)
        n = games.size
        torch = _torch_for_device()
        ply_off = np.zeros(n + 1, np.uint32)
        _check(self.L.sc_selfplay_encode_traces(self.h, n, _p(games), 0, 0, None, _p(ply_off), None, None, None, None, None,
                                                None, None))
        win = np.zeros(n, np.float32)
        info = TraceInfo()
        for i, g in enumerate(games):
            _check(self.L.sc_selfplay_get_trace(self.h, int(g), C.byref(info), None, None, None, None, None, None, None))
            win[i] = {1: 1.0, 0: -1.0}.get(info.winner, 0.0) if info.has_outcome else 0.0
        out, args = _device_outputs(torch, self.device, int(ply_off[n]), n, layout, dist)
        stream = torch.cuda.current_stream(self.device)
        _check(self.L.sc_selfplay_encode_traces(self.h, n, _p(games), int(bool(apply_mirror)), args[0], C.c_void_p(stream.cuda_stream),
                                                _p(ply_off), *args[1:]))
        return _finish_outputs(torch, out, ply_off, win, apply_mirror, self.device)

    def write_trace(self, game, path):
        _check(self.L.sc_selfplay_write_trace_json(self.h, game, path.encode()))

    def stream_traces(self, path_of, chunk=None):
        """The loop of lib/sc-selfplay (src/main.rs:235-238 writes each game's file when it ends): plays every game of the
        handle and writes `path_of(game_id)` as games finish, from a handle created with a trace ring and trace_hold=True.
        The next ply's simulation steps are enqueued BEFORE the finished games' traces are fetched and written: a reported
        row is final, it is read while the GPU searches.  -> number of files written."""
        chunk = chunk or self.cfg.rollout_num
        written = 0
        self.enqueue(chunk)
        while True:
            fin = self.poll()
            active = self.stats()["games_active"]
            if active:
                self.enqueue(chunk)
            for g in fin:
                self.write_trace(g, path_of(self.cfg.first_game_id + g))
                written += 1
            if not active and not fin:
                return written

    def tree(self, slot, cap=1 << 20):
        n = self.L.sc_selfplay_get_tree(self.h, slot, 0, None, None, None, None, None, None, None)
        if n < 0:
            _check(n)
        n = min(n, cap)
        out = dict(n=np.zeros(n, np.int32), q=np.zeros(n, np.float32), uct=np.zeros(n, np.float32),
                   prior=np.zeros(n, np.float32), move=np.zeros(n, np.uint16), first_child=np.zeros(n, np.int32),
                   n_child=np.zeros(n, np.int32))
        r = self.L.sc_selfplay_get_tree(self.h, slot, n, _p(out["n"]), _p(out["q"]), _p(out["uct"]), _p(out["prior"]),
                                        _p(out["move"]), _p(out["first_child"]), _p(out["n_child"]))
        if r < 0:
            _check(r)
        return out

    def debug_cycles(self, enable=True, read=False):
        """sc_selfplay_debug_cycles: switch the stamps on / read those of the last launch -> uint64[n_slots, 32] (or None)"""
        out = np.zeros((self.cfg.n_slots, 32), np.uint64) if read else None
        _check(self.L.sc_selfplay_debug_cycles(self.h, int(enable), _p(out)))
        return out

    def slot(self, slot):
        ply, sim, st, plen = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        gid = C.c_uint64(0)
        path = np.zeros(1024, np.int32)
        _check(self.L.sc_selfplay_get_slot(self.h, slot, C.byref(ply), C.byref(sim), C.byref(st), C.byref(gid), _p(path),
                                           C.byref(plen)))
        return dict(ply=ply.value, sim=sim.value, status=st.value, game_id=gid.value, path=path[:plen.value].copy())

    def set_noise(self, slot, noise):
        noise = np.ascontiguousarray(noise, np.float32)
        _check(self.L.sc_selfplay_set_noise(self.h, slot, _p(noise), noise.size))

    def get_noise(self, slot, n):
        out = np.zeros(MAX_MOVES, np.float32)
        _check(self.L.sc_selfplay_get_noise(self.h, slot, _p(out), MAX_MOVES))
        return out[:n]

    def set_position(self, slot, moves):
        mv = np.asarray([uci_move(m) if isinstance(m, str) else int(m) for m in moves], np.uint16)
        if mv.size == 0:
            mv = np.zeros(1, np.uint16)
        _check(self.L.sc_selfplay_set_position(self.h, slot, _p(mv), len(moves)))


def find_max(values, device=0):
    """sc_debug_find_max: (one-round result or -2, four-round result) of the descent's arg-max on `values`"""
    v = np.ascontiguousarray(values, np.float32)
    out = np.zeros(2, np.int32)
    _check(lib().sc_debug_find_max(device, _p(v), v.size, _p(out)))
    return int(out[0]), int(out[1])


def choose_child(n_act, nc, temperature, u, tie_random=False, device=0):
    """sc_debug_choose_child: (choice [n] int32, total [n] float32) of the end-of-ply move choice on n cases;
    n_act [n][224] visit counts, nc / temperature / u one value per case"""
    nc = np.ascontiguousarray(nc, np.int32)
    n = nc.size
    n_act = np.ascontiguousarray(n_act, np.int32)
    temperature = np.ascontiguousarray(temperature, np.float32)
    u = np.ascontiguousarray(u, np.float32)
    if n_act.shape != (n, MAX_MOVES) or temperature.shape != (n,) or u.shape != (n,):
        raise ValueError("choose_child: n_act must be [n][224], nc / temperature / u [n]")
    choice = np.zeros(n, np.int32)
    total = np.zeros(n, np.float32)
    _check(lib().sc_debug_choose_child(device, n, _p(n_act), _p(nc), _p(temperature), _p(u), int(tie_random), _p(choice), _p(total)))
    return choice, total


def runtime_flags():
    return int(lib().sc_runtime_flags())


def enqueue_interleaved(handles, n_sims):
    """n simulation steps on several SelfPlay handles (own_stream=True), interleaved step by step"""
    arr = (C.c_void_p * len(handles))(*[h.h for h in handles])
    _check(lib().sc_selfplay_enqueue_interleaved(arr, len(handles), n_sims))


def write_trace_json(path, trace):
    """sc_trace_write_json on a trace dict (no GPU needed)."""
    steps = trace["steps"]
    ns = len(steps)
    info = TraceInfo()
    info.n_steps = ns
    oc = trace.get("outcome")
    info.has_outcome = int(oc is not None)
    inv_t = {v: k for k, v in TERMINATION.items()}
    info.termination = inv_t[oc["termination"]] if oc else 0
    info.winner = {"White": 1, "Black": 0, None: -1}[oc["winner"]] if oc else -1
    sm = np.asarray([uci_move(s[0]) for s in steps] + [0], np.uint16)
    sq = np.asarray([s[1] for s in steps] + [0], np.float32)
    co = np.zeros(ns + 2, np.int32)
    co[1:ns + 1] = np.cumsum([len(s[2]) for s in steps])
    ch = [c for s in steps for c in s[2]]
    info.n_children_total = len(ch)
    cm = np.asarray([uci_move(c[0]) for c in ch] + [0], np.uint16)
    cn = np.asarray([c[1] for c in ch] + [0], np.int32)
    cq = np.asarray([c[2] for c in ch] + [0], np.float32)
    cu = np.asarray([c[3] for c in ch] + [0], np.float32)
    _check(lib().sc_trace_write_json(path.encode(), C.byref(info), _p(sm), _p(sq), _p(co), _p(cm), _p(cn), _p(cq), _p(cu)))
