"""Trace files read on the device, the checks that need no GPU: the eight entry points are declared, bound and exported with equal
arity, the Python names live in scamd.traces only, the codes of the header are the module's, sc_traces_read finds bad offsets
before it looks for a device and refuses without one."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from support import ROOT, scamd_built  # noqa: F401

ENTRY_POINTS = (("sc_traces_read", 5), ("sc_traces_destroy", 1), ("sc_traces_count", 1), ("sc_traces_summary", 8), ("sc_traces_get", 10),
                ("sc_traces_fen", 4), ("sc_traces_encode_device", 14), ("sc_traces_last_timing", 2))


@pytest.fixture(scope="module")
def traces(scamd):
    import scamd.traces as m
    return m


def _header():
    return open(os.path.join(ROOT, "include", "sc_engine.h")).read()


def test_symbols_are_declared_bound_and_exported(scamd):
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", scamd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TW"}
    for name, arity in ENTRY_POINTS:
        m = re.search(rf"\b{name}\s*\((.*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == arity == len(scamd.binding.ABI[name][1]), name
        assert name in exported, name
    assert "typedef struct sc_traces sc_traces;" in hdr


def test_names_live_in_the_submodule_only(scamd, traces):
    for name in ("read", "Traces", "encode_traces_torch", "batches"):
        assert callable(getattr(traces, name)) and not hasattr(scamd, name), name


def test_codes_are_the_headers(traces):
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define SC_TRACE_ERR_(\w+) (\d+)", _header())}
    assert len(codes) == 10 and sorted(codes.values()) == list(range(1, 11))
    for name, code in codes.items():
        assert getattr(traces, "ERR_" + name) == code and traces.ERR_NAMES[code] == name
    import trace_text_ref as ref
    assert all(getattr(ref, name) == code for name, code in codes.items())
    assert ref.TERMINATION_NAMES == traces.TERMINATION_NAMES
    src = open(os.path.join(ROOT, "smart-chess-rust_amd", "csrc", "trace_json.hpp")).read()
    assert all(f'"{t}"' in src for t in traces.TERMINATION_NAMES[1:])


def test_bad_offsets_are_found_before_a_device_is_looked_for(scamd):
    L = scamd.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    h = C.c_void_p(77)
    text = b'{"steps":[]}' * 2
    assert L.sc_traces_read(0, 2, text, p(np.array([0, 13, 12], np.uint64)), C.byref(h)) == -1 and not h.value
    assert "monotonic" in L.sc_last_error().decode()
    assert L.sc_traces_read(0, 1, text, p(np.array([0, 1 << 32], np.uint64)), C.byref(h)) == -1 and "2^32" in L.sc_last_error().decode()
    assert L.sc_traces_read(0, -1, text, p(np.array([0], np.uint64)), C.byref(h)) == -1
    assert L.sc_traces_read(0, 1, text, None, C.byref(h)) == -1 and L.sc_traces_read(0, 1, text, p(np.array([0, 12], np.uint64)), None) == -1
    assert L.sc_traces_count(None) == -1 and L.sc_traces_fen(None, 0, None, 0) == -1
    L.sc_traces_destroy(None)


def test_refuses_without_a_device(scamd, traces):
    L = scamd.lib()
    if L.sc_device_count() > 0:
        pytest.skip("a GPU is present")
    h = C.c_void_p()
    off = np.array([0, 12], np.uint64)
    assert L.sc_traces_read(0, 1, b'{"steps":[]}', off.ctypes.data_as(C.c_void_p), C.byref(h)) == -3 and not h.value
    assert "no HIP device" in L.sc_last_error().decode()
    with pytest.raises(scamd.EngineError, match="no HIP device"):
        traces.read([b'{"steps":[]}'])


def test_batches_split_a_file_list(traces, tmp_path, monkeypatch):
    paths = []
    for i, size in enumerate((10, 20, 100, 5, 5, 30)):
        p = tmp_path / f"{i}.json"
        p.write_bytes(b" " * size)
        paths.append(str(p))
    monkeypatch.setattr(traces, "read", lambda group, device=0: ("set", len(group)))
    got = [g for _, g in traces.batches(paths, max_bytes=40)]
    assert got == [paths[0:2], paths[2:3], paths[3:6]]          # the file above max_bytes alone
    assert [g for _, g in traces.batches(paths, max_bytes=1 << 30)] == [paths]
    assert list(traces.batches([], max_bytes=40)) == []
