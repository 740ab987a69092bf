"""What the test files share: the two `scamd` fixtures, device buffers on the engine's HIP runtime (no torch), host pointers,
and the device calls of the encoders (run_san, run_steps) with the exact comparison of their tensors.
A fixture imported into a test module is that module's own fixture.  Two fixtures here are named `scamd` and two `dev`: a test file imports
exactly one of each pair -- with both imported, pytest silently keeps one of them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


class Dev:
    """device buffers (pre-filled with `fill`) and one non-default stream on the engine's HIP runtime"""

    def __init__(self, scamd, fill=0x5a):
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


def open_dev(scamd, fill=0x5a):
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


def run_san(scamd, san, dev, games, mirror=False, layout=0, skip=()):
    """sc_encode_san_device on a non-default stream into buffers pre-filled with 0x5a (outputs named in `skip` are passed as
    NULL); read back after synchronising that stream.  games: movetext strings or token arrays"""
    tokens, off = san.pack_tokens(games)
    n, P = len(games), int(off[-1])
    o = {k: (None if k in skip else dev.alloc(nb)) for k, nb in _sizes(P, layout).items()}
    o["status"] = dev.alloc(max(n, 1) * 4)
    rc = scamd.lib().sc_encode_san_device(None, 0, n, _p(tokens if tokens.size else np.zeros(1, np.uint64)), _p(off), int(mirror), layout,
                                          dev.stream, *[o[k] for k in TENSORS], o["moves"], o["status"])
    assert rc == 0, scamd.lib().sc_last_error().decode()
    dev.sync()
    r = _read(dev, o, P, n, layout)
    r["ply_off"] = off
    return r


def run_steps(scamd, dev, steps, mirror=False, layout=0):
    """the tensor yardstick: sc_encode_steps_device on moves and children"""
    mv, off, cm, cn, coff = scamd.pack_steps(steps)
    n, P = len(steps), int(off[-1])
    o = {k: dev.alloc(nb) for k, nb in _sizes(P, layout).items() if k != "moves"}
    o["status"] = dev.alloc(max(n, 1) * 4)
    rc = scamd.lib().sc_encode_steps_device(None, 0, n, _p(mv), _p(off), _p(cm), _p(cn), _p(coff), int(mirror), layout, dev.stream,
                                            *[o[k] for k in TENSORS], o["status"])
    assert rc == 0, scamd.lib().sc_last_error().decode()
    dev.sync()
    r = _read(dev, o, P, n, layout)
    r["moves"] = mv[:P]
    return r


def assert_bit_equal(got, ref, keys=TENSORS + ("moves",), rows=None):
    for k in keys:
        if k in got:
            a, b = (got[k], ref[k]) if rows is None else (got[k][rows], ref[k][rows])
            assert a.dtype == b.dtype and a.shape == b.shape, k
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), k
