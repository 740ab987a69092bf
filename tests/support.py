"""The package, the device and processes -- what a test needs beyond chess and data (tests/helpers.py, tests/lines.py):
  ROOT, GOLD, INST / IDS                     the repository, tests/golden, the four instantiations of the tower
  scamd_gpu, scamd_built                     the two `scamd` fixtures
  rules_host                                 the `H` fixture: the engine's rules compiled for the host
  Dev, open_dev, dev_per_test, dev_per_module, FILL, untouched, _p
                                             device buffers on the engine's HIP runtime (no torch), pre-filled with FILL; host pointers
  engine_from_state                          an Engine from a state dict, through a weight blob
  alloc_outputs, run_san, run_steps, assert_bit_equal
                                             the encoders' output buffers and device calls, the exact comparison of their tensors
  run_torch_child                            a script that imports torch first, in a process of its own
A fixture imported into a test module is that module's own fixture.  Two fixtures here are named `scamd` and two `dev`: a test file imports
exactly one of each pair -- with both imported, pytest silently keeps one of them."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
INST = [(128, "bf16"), (256, "bf16"), (128, "fp8"), (256, "fp8")]   # (channels, precision) of the tower's four instantiations
IDS = [f"{ch}_{p}" for ch, p in INST]
FILL = 0x5a   # every byte of a fresh device buffer
H2D, D2H = 1, 2   # hipMemcpyHostToDevice, hipMemcpyDeviceToHost


@pytest.fixture(scope="module", name="scamd")
def scamd_gpu():
    """the package, for the GPU tests: a machine without a device fails them (there is no fallback)"""
    sys.path.insert(0, os.path.join(ROOT, "smart-chess-rust_amd"))
    import scamd as m
    if m.lib().sc_device_count() <= 0:
        pytest.fail("no MI355X visible: the HIP path cannot be tested (and there is no fallback)")
    return m


@pytest.fixture(scope="module", name="scamd")
def scamd_built():
    """the package, for the ABI tests: built first, no device needed"""
    sys.path.insert(0, os.path.join(ROOT, "smart-chess-rust_amd"))
    import build as scbuild
    scbuild.build()
    import scamd as m
    return m


@pytest.fixture(scope="module", name="H")
def rules_host():
    """the engine's rules source compiled for the host (lib/libsc_rules_host.so, rebuilt when its sources are newer), through ctypes"""
    PKG = os.path.join(ROOT, "smart-chess-rust_amd")
    so = os.path.join(PKG, "lib", "libsc_rules_host.so")
    src = os.path.join(PKG, "csrc", "rules_host_api.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(os.path.join(PKG, "csrc", f))
                                                           for f in ("rules_host_api.cpp", "chess_rules.hpp", "chess_history.hpp")):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src])
    L = C.CDLL(so)
    L.sct_new.restype = C.c_void_p
    L.sct_perft.restype = C.c_uint64
    L.sct_pos_hash.restype = C.c_uint64
    L.sct_rng.restype = C.c_uint64
    L.sct_key.restype = C.c_uint64
    L.sct_key_full.restype = C.c_uint64
    L.sct_key.argtypes = [C.c_void_p]
    L.sct_key_full.argtypes = [C.c_void_p]
    L.sct_rng.argtypes = [C.c_uint64] * 5
    for n in ("sct_free", "sct_reset", "sct_push", "sct_pop", "sct_encode", "sct_synth_eval"):
        getattr(L, n).restype = None
    L.sct_set_fen.argtypes = [C.c_void_p, C.c_char_p]
    L.sct_push.argtypes = [C.c_void_p, C.c_uint16]
    L.sct_move_index.argtypes = [C.c_uint16, C.c_int]
    for n in ("sct_free", "sct_reset", "sct_pop", "sct_pos_hash", "sct_turn"):
        getattr(L, n).argtypes = [C.c_void_p]
    L.sct_legal_moves.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.sct_perft.argtypes = [C.c_void_p, C.c_int]
    L.sct_is_repetition.argtypes = [C.c_void_p, C.c_int]
    L.sct_outcome.argtypes = [C.c_void_p, C.c_void_p]
    L.sct_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.sct_board_diff_legal.argtypes = [C.c_void_p, C.c_void_p]
    L.sct_synth_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    return L


class Dev:
    """device buffers (pre-filled with `fill`) and one non-default stream on the engine's HIP runtime"""

    def __init__(self, scamd, fill=FILL):
        self.fill = fill
        self.hip = scamd.hip_runtime()
        self.bufs = []
        s = C.c_void_p()
        assert self.hip.hipStreamCreate(C.byref(s)) == 0
        self.stream = s

    def alloc(self, nbytes, fill=None):
        fill = self.fill if fill is None else fill
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(int(nbytes), 1)) == 0
        assert self.hip.hipMemset(p, fill, max(int(nbytes), 1)) == 0   # garbage: every byte the call owns must be written
        self.bufs.append(p)
        return p

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        if a.nbytes:
            assert self.hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, H2D) == 0
        return p

    def read(self, p, shape, dtype):
        out = np.empty(shape, dtype)
        if out.nbytes:
            assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), p, out.nbytes, D2H) == 0
        return out

    def sync(self):
        assert self.hip.hipStreamSynchronize(self.stream) == 0

    def close(self):
        self.sync()
        for p in self.bufs:
            self.hip.hipFree(p)
        self.hip.hipStreamDestroy(self.stream)


def open_dev(scamd, fill=FILL):
    d = Dev(scamd, fill)
    yield d
    d.close()


@pytest.fixture(name="dev")
def dev_per_test(scamd):
    yield from open_dev(scamd)


@pytest.fixture(scope="module", name="dev")
def dev_per_module(scamd):
    yield from open_dev(scamd)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def untouched(a, fill=FILL):
    """every byte of a still holds the fill of its device buffer"""
    return (np.ascontiguousarray(a).view(np.uint8) == fill).all()


def engine_from_state(scamd, tmp_path, sd, nb, C, prec, skip=()):
    """an Engine of nb blocks, C channels and precision prec on the weights sd, written as a blob and loaded from it; skip: the
    names that tower_ref.representable leaves out"""
    import scw
    import tower_ref as tw
    tw.representable(sd, prec, skip)
    path = str(tmp_path / "w.scw")
    scw.write_scw(path, sd, nb, C)
    eng = scamd.Engine(n_res_blocks=nb, channels=C, weights=path, precision=prec)   # debug() sizes its output by these
    assert eng.precision == prec and eng.channels == C
    return eng


# ------------------------------------------------------------------ the encoders' device calls
TENSORS = ("boards", "meta", "dist", "dist_legal", "legal_idx", "n_legal")


def _sizes(P, layout):
    P1 = max(P, 1)
    return dict(boards=P1 * 7168 * (4 if layout else 1), meta=P1 * 28, dist=P1 * 4672 * 4, dist_legal=P1 * 224 * 4, legal_idx=P1 * 448,
                n_legal=P1 * 4, moves=P1 * 2)


def _read(dev, o, P, n, layout):
    shapes = dict(boards=((P, 112, 8, 8) if layout else (P, 8, 8, 112), np.float32 if layout else np.int8),
                  meta=((P, 7), np.float32 if layout else np.int32), dist=((P, 4672), np.float32), dist_legal=((P, 224), np.float32),
                  legal_idx=((P, 224), np.uint16), n_legal=((P,), np.int32), moves=((P,), np.uint16), status=((n,), np.int32))
    return {k: dev.read(o[k], *shapes[k]) for k in o if o[k] is not None}


def alloc_outputs(dev, P, n, layout, skip=("moves",)):
    """the encoders' output buffers for P plies of n games, fresh from dev.alloc, and `status`; None for the names in `skip`"""
    o = {k: (None if k in skip else dev.alloc(nb)) for k, nb in _sizes(P, layout).items()}
    o["status"] = dev.alloc(max(n, 1) * 4)
    return o


def run_san(scamd, san, dev, games, mirror=False, layout=0, skip=()):
    """sc_encode_san_device on a non-default stream into buffers pre-filled with 0x5a (outputs named in `skip` are passed as
    NULL); read back after synchronising that stream.  games: movetext strings or token arrays"""
    tokens, off = san.pack_tokens(games)
    n, P = len(games), int(off[-1])
    o = alloc_outputs(dev, P, n, layout, skip)
    rc = scamd.lib().sc_encode_san_device(None, 0, n, _p(tokens if tokens.size else np.zeros(1, np.uint64)), _p(off), int(mirror), layout,
                                          dev.stream, *[o[k] for k in TENSORS], o["moves"], o["status"])
    assert rc == 0, scamd.lib().sc_last_error().decode()
    dev.sync()
    r = _read(dev, o, P, n, layout)
    r["ply_off"] = off
    return r


def run_steps(scamd, dev, steps, mirror=False, layout=0):
    """the tensor yardstick: sc_encode_steps_device on moves and children, on a non-default stream; read back after synchronising
    that stream"""
    mv, off, cm, cn, coff = scamd.pack_steps(steps)
    n, P = len(steps), int(off[-1])
    o = alloc_outputs(dev, P, n, layout)
    rc = scamd.lib().sc_encode_steps_device(None, 0, n, _p(mv), _p(off), _p(cm), _p(cn), _p(coff), int(mirror), layout, dev.stream,
                                            *[o[k] for k in TENSORS], o["status"])
    assert rc == 0, scamd.lib().sc_last_error().decode()
    dev.sync()
    r = _read(dev, o, P, n, layout)
    r["moves"], r["ply_off"] = mv[:P], off
    return r


def assert_bit_equal(got, ref, keys=TENSORS + ("moves",), rows=None):
    for k in keys:
        if k in got:
            a, b = (got[k], ref[k]) if rows is None else (got[k][rows], ref[k][rows])
            assert a.dtype == b.dtype and a.shape == b.shape, k
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), k


# ------------------------------------------------------------------ torch, in a process of its own
def run_torch_child(tmp_path, script, *args, timeout=600):
    """write `script` to tmp_path/child.py, run it with `args` in a fresh interpreter (this process keeps its own HIP runtime; the
    script imports torch before scamd) and return what its last line of output says, as JSON"""
    path = tmp_path / "child.py"
    path.write_text(script)
    r = subprocess.run([sys.executable, str(path), *args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])
