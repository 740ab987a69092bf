"""ctypes binding of include/sc_engine.h (libsc_engine.so): the ABI table, library loading, the helpers of the other modules."""
import ctypes as C
import os

# see INTEGRATION.md: kernel arguments in device memory (must precede HIP runtime initialisation)
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SC_ENGINE_LIB: developer override (experiment builds of the same library); there is still no CPU fallback
_LIB_PATH = os.environ.get("SC_ENGINE_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libsc_engine.so")

MAX_MOVES = 224
PLY_BYTES = 7168 + 28 + 4 * MAX_MOVES + 2 * MAX_MOVES + 4 + 4   # one ply of the compact training tensors (replay.py): 8 548
TERMINATION = {0: None, 1: "Checkmate", 2: "Stalemate", 3: "InsufficientMaterial", 4: "SeventyfiveMoves",
               5: "FivefoldRepetition", 6: "FiftyMoves", 7: "ThreefoldRepetition"}
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
    "sc_fen_parse": (_i, [C.c_char_p, C.c_size_t, _vp]),
    "sc_positions_from_fen": (_i, [_i, _i, _vp, C.POINTER(_vp), _vp]),
    "sc_positions_destroy": (None, [_vp]),
    "sc_positions_count": (_i, [_vp]),
    "sc_positions_status": (_i, [_vp, _i]),
    "sc_positions_fen": (_i, [_vp, _i, C.c_char_p, _i]),
    "sc_perft": (_i, [_i, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_perft_last_timing": (_i, [C.POINTER(_f), C.POINTER(_f)]),
    "sc_encode_positions_from": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_encode_steps_device_from": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_encode_san_device_from": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_selfplay_set_position_from": (_i, [_vp, _i, _vp, _i, _vp, _i]),
    "sc_search_from": (_i, [_vp, _vp, _i, _vp, _i, _i, _f, _i, C.c_uint64, _i, _vp, _vp, _vp, _vp, _vp]),
    "sc_selfplay_get_fen": (_i, [_vp, _i, C.c_char_p, _i]),
    "sc_selfplay_set_openings_from": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "sc_selfplay_get_opening_fen": (_i, [_vp, _i, C.c_char_p, _i]),
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
    "sc_selfplay_set_match": (_i, [_vp, _vp, _vp, C.c_uint64, C.c_uint64, _i]),
    "sc_selfplay_match_tally": (_i, [_vp, _vp]),
    "sc_selfplay_set_external": (_i, [_vp, _vp, C.c_uint64, _i]),
    "sc_selfplay_external_search": (_i, [_vp]),
    "sc_selfplay_external_wait": (_i, [_vp, _i, _vp, _vp, _vp, _vp, C.c_uint64, _vp, _vp, C.c_uint32, _vp]),
    "sc_selfplay_push_moves": (_i, [_vp, _i, _vp, _vp, _vp]),
    "sc_selfplay_advance": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "sc_selfplay_set_openings": (_i, [_vp, _i, _vp, _vp, _vp]),
    "sc_selfplay_get_opening": (_i, [_vp, _i, _vp, _i]),
    "sc_selfplay_enable_timing": (_i, [_vp, _i]),
    "sc_selfplay_timing": (_i, [_vp, _i, C.POINTER(_f), C.POINTER(_f), C.POINTER(_i64)]),
    "sc_selfplay_launches_per_step": (_i, [_vp]),
    "sc_selfplay_get_trace": (_i, [_vp, _i, C.POINTER(TraceInfo), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_selfplay_write_trace_json": (_i, [_vp, _i, C.c_char_p]),
    "sc_selfplay_write_pgn": (_i, [_vp, _i, _vp, C.c_char_p, _i, C.c_char_p, C.c_char_p, C.c_char_p]),
    "sc_selfplay_get_tree": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_selfplay_report": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_selfplay_report_last_timing": (_i, [C.POINTER(_f), C.POINTER(_f)]),
    "sc_selfplay_get_slot": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_selfplay_set_noise": (_i, [_vp, _i, _vp, _i]),
    "sc_selfplay_get_noise": (_i, [_vp, _i, _vp, _i]),
    "sc_selfplay_set_position": (_i, [_vp, _i, _vp, _i]),
    "sc_encode_steps_last_timing": (_i, [C.POINTER(_f), C.POINTER(_f)]),
    "sc_encode_steps": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_encode_steps_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_san_tokenize": (_i, [C.c_char_p, C.c_size_t, _vp, C.c_uint32, _vp]),
    "sc_encode_san_device": (_i, [_vp, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_moves_to_san_device": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp]),
    "sc_moves_to_san_device_from": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_san_format": (_i, [_vp, C.c_uint32, _i, _i, C.c_char_p, C.c_char_p, C.c_size_t]),
    "sc_traces_read": (_i, [_i, _i, _vp, _vp, C.POINTER(_vp)]),
    "sc_traces_destroy": (None, [_vp]),
    "sc_traces_count": (_i, [_vp]),
    "sc_traces_summary": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_traces_get": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_traces_fen": (_i, [_vp, _i, C.c_char_p, _i]),
    "sc_traces_encode_device": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_traces_last_timing": (_i, [C.POINTER(_f), C.POINTER(_f)]),
    "sc_trace_format_f32": (_i, [_i, _vp, _vp, _vp]),
    "sc_traces_format": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_uint64, _vp]),
    "sc_traces_format_last_timing": (_i, [C.POINTER(_f), C.POINTER(_f)]),
    "sc_selfplay_traces_json": (_i, [_vp, _i, _vp, _vp, C.c_uint64, _vp]),
    "sc_selfplay_write_traces_json": (_i, [_vp, _i, _vp, _vp]),
    "sc_selfplay_encode_traces": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_forward_device": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "sc_score_positions": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_compare_engines": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_gather_batch": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_merge_positions_workspace": (_i, [_i, C.POINTER(C.c_size_t)]),
    "sc_merge_positions": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, C.c_size_t, _vp] + [_vp] * 10),
    "sc_trace_write_json": (_i, [C.c_char_p, C.POINTER(TraceInfo), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_move_uci": (_i, [C.c_uint16, C.c_char_p]),
    "sc_move_index": (_i, [C.c_uint16, _i]),
}

_lib = None
_engine_hip = []   # libamdhip64 file(s) libsc_engine.so bound to when it was loaded


def hip_runtime_files():
    """the distinct libamdhip64 files mapped into this process (/proc/self/maps)"""
    found = set()
    with open("/proc/self/maps") as f:
        for ln in f:
            parts = ln.split(None, 5)
            if len(parts) == 6 and os.path.basename(parts[5].strip()).startswith("libamdhip64"):
                found.add(os.path.realpath(parts[5].strip()))
    return sorted(found)


def lib_path():
    return _LIB_PATH


def lib():
    """Loads libsc_engine.so; raises EngineError (never falls back) when it is missing."""
    global _lib, _engine_hip
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
    new = set(hip_runtime_files()) - before
    _engine_hip = sorted(new or before)
    for name, (res, args) in ABI.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


_HIP_ABI = {
    "hipMalloc": [C.POINTER(_vp), C.c_size_t],
    "hipFree": [_vp],
    "hipMemcpy": [_vp, _vp, C.c_size_t, _i],
    "hipMemset": [_vp, _i, C.c_size_t],
    "hipStreamCreate": [C.POINTER(_vp)],
    "hipStreamSynchronize": [_vp],
    "hipStreamDestroy": [_vp],
    "hipEventCreate": [C.POINTER(_vp)],
    "hipEventRecord": [_vp, _vp],
    "hipEventElapsedTime": [C.POINTER(C.c_float), _vp, _vp],
    "hipEventDestroy": [_vp],
}
_hip = None


def hip_runtime():
    """ctypes handle of the HIP runtime libsc_engine.so uses (device buffers for the *_device entry points without torch): one per
    process, with the argument types of the runtime calls the project makes through it"""
    global _hip
    if _hip is None:
        lib()
        if len(_engine_hip) != 1:
            raise EngineError(f"cannot tell which HIP runtime libsc_engine.so uses: {_engine_hip}")
        H = C.CDLL(_engine_hip[0])
        for name, args in _HIP_ABI.items():
            getattr(H, name).argtypes = args
        _hip = H
    return _hip


def _check(rc):
    if rc != 0:
        e = EngineError(f"libsc_engine error {rc}: {lib().sc_last_error().decode()}")
        e.code = rc
        raise e


def _count(n):
    """a negative return is an error code, anything else a count"""
    if n < 0:
        _check(n)
    return n


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _tp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(torch, device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class _Handle:
    """owner of a library handle `h`: destroyed once, by close() or when the object is collected"""
    _destroy = None   # name of the sc_*_destroy entry point

    def close(self):
        if getattr(self, "h", None):
            getattr(self.L, self._destroy)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def move_uci(m):
    buf = C.create_string_buffer(8)
    lib().sc_move_uci(int(m), buf)
    return buf.value.decode()


def uci_move(s):
    promo = {"n": 2, "b": 3, "r": 4, "q": 5}
    f = (ord(s[1]) - 49) * 8 + ord(s[0]) - 97
    t = (ord(s[3]) - 49) * 8 + ord(s[2]) - 97
    return f | (t << 6) | ((promo[s[4]] if len(s) > 4 else 0) << 12)


def _moves(moves):
    """moves (UCI strings or ints) -> uint16 array, one placeholder element if there are none: the length is passed separately"""
    return np.asarray([uci_move(m) if isinstance(m, str) else int(m) for m in moves] or [0], np.uint16)


def encode_move(turn_white, move):
    """libsmartchess.chess_encode_move(turn, move) (reference src/lib.rs:37-44); no GPU needed"""
    return int(lib().sc_move_index(uci_move(move) if isinstance(move, str) else int(move), int(bool(turn_white))))


_torch_checked = None


def _torch(cached=False):
    """torch, after checking that there is a GPU and that torch shares the engine's HIP runtime: device pointers must not cross
    between two runtimes.  cached: the first such call checks, the later ones return its result and do not read /proc/self/maps again"""
    global _torch_checked
    if cached and _torch_checked is not None:
        return _torch_checked
    if lib().sc_device_count() <= 0:
        raise EngineError("no HIP device available: libsc_engine has no CPU fallback")
    import torch
    files = hip_runtime_files()
    if len(files) > 1:
        raise EngineError(f"two HIP runtimes are loaded ({', '.join(files)}): torch was imported after scamd loaded "
                          "libsc_engine.so -- import torch before scamd")
    if cached:
        _torch_checked = torch
    return torch


def runtime_flags():
    return int(lib().sc_runtime_flags())


def encode_steps_last_timing():
    """(kernel ms, whole-call ms) of this thread's last sc_encode_steps"""
    a, b = C.c_float(0), C.c_float(0)
    lib().sc_encode_steps_last_timing(C.byref(a), C.byref(b))
    return a.value, b.value
