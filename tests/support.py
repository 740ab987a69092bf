"""What the test files share: the two `scamd` fixtures, device buffers on the engine's HIP runtime (no torch), host pointers.
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
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        self.hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        self.hip.hipStreamDestroy.argtypes = [C.c_void_p]
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
