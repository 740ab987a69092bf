"""Trace files written on the device, the checks that need no GPU: the five entry points are declared, bound and exported with
equal arity, the number formatter of the kernels (csrc/trace_fmt.hpp through sc_trace_format_f32: the same source, integer
arithmetic only) equals the reference's pretty on the float edge set and 20 000 random patterns and never needs more than 24
bytes, sc_traces_format finds argument errors before it looks for a device and refuses without one."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from support import ROOT, scamd_built  # noqa: F401

import trace_write_ref as ref

ENTRY_POINTS = (("sc_trace_format_f32", 4), ("sc_traces_format", 17), ("sc_selfplay_traces_json", 6), ("sc_selfplay_write_traces_json", 4),
                ("sc_traces_format_last_timing", 2))


def test_symbols_are_declared_bound_and_exported(scamd):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sc_engine.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", scamd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TW"}
    for name, arity in ENTRY_POINTS:
        m = re.search(rf"\b{name}\s*\((.*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == arity == len(scamd.binding.ABI[name][1]), name
        assert name in exported, name


def test_python_names(scamd):
    import scamd.traces as traces
    for name in ("format", "write", "pack_traces"):
        assert callable(getattr(traces, name)) and not hasattr(scamd, name), name
    assert callable(scamd.SelfPlay.traces_json) and callable(scamd.SelfPlay.write_traces)


def _format(scamd, vals):
    vals = np.ascontiguousarray(vals, np.float32)
    text, length = np.full((vals.size, 24), 0x5a, np.uint8), np.zeros(vals.size, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert scamd.lib().sc_trace_format_f32(vals.size, p(vals), p(text), p(length)) == 0
    return text, length


def test_formatter_equals_the_reference(scamd):
    bits = np.concatenate([ref.edge_bits(), np.random.default_rng(12).integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32)])
    vals = ref.f32(bits)
    text, length = _format(scamd, vals)
    assert int(length.max()) <= 24 and int(length.min()) >= 3
    for i, v in enumerate(vals):
        want = ref.pretty(v).encode()
        assert text[i, :length[i]].tobytes() == want, (hex(int(bits[i])), want)
        assert (text[i, length[i]:] == 0x5a).all()      # nothing behind the text
    text, length = _format(scamd, [ref.f32(0xB77FFFFF)])   # one below 2^-16
    assert text[0, :length[0]].tobytes() == b"-0.000015258788153005298" and length[0] == 24


def test_formatter_arguments(scamd):
    L = scamd.lib()
    assert L.sc_trace_format_f32(0, None, None, None) == 0
    assert L.sc_trace_format_f32(-1, None, None, None) == -1 and L.sc_trace_format_f32(1, None, None, None) == -1


def _call(L, n, info, step_off, child_off, text_off, step_move=None, step_q=None, child=(None,) * 4, open_off=None, opening=None):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return L.sc_traces_format(0, n, info, p(step_off), p(step_move), p(step_q), p(child_off), *[p(c) for c in child], p(open_off), p(opening),
                              None, None, 0, p(text_off))


def test_argument_errors_are_found_before_a_device_is_looked_for(scamd):
    L = scamd.lib()
    info = (scamd.binding.TraceInfo * 2)()
    info[0].n_steps, info[1].n_steps = 1, 0
    u32 = lambda *v: np.array(v, np.uint32)
    off = np.zeros(3, np.uint64)
    mv, q = np.zeros(4, np.uint16), np.zeros(4, np.float32)
    assert _call(L, -1, info, u32(0), u32(0), off) == -1
    assert _call(L, 2, info, u32(0, 1, 1), u32(0, 0), None) == -1                          # no text_off
    assert _call(L, 2, None, u32(0, 1, 1), u32(0, 0), off) == -1                           # no info
    assert _call(L, 2, info, u32(0, 2, 1), u32(0, 0, 0), off, mv, q) == -1 and "monotonic" in L.sc_last_error().decode()
    assert _call(L, 2, info, u32(0, 1, 1), u32(0, 225), off, mv, q) == -1 and "224" in L.sc_last_error().decode()
    assert _call(L, 2, info, u32(0, 2, 2), u32(0, 0, 0), off, mv, q) == -1 and "n_steps" in L.sc_last_error().decode()
    assert _call(L, 2, info, u32(0, 1, 1), u32(0, 0), off) == -1                           # steps without their arrays
    assert _call(L, 2, info, u32(0, 1, 1), u32(0, 1), off, mv, q) == -1                    # children without their arrays
    assert _call(L, 2, info, u32(0, 1, 1), u32(0, 0), off, mv, q, open_off=u32(0, 2, 1), opening=mv) == -1
    assert "open_off" in L.sc_last_error().decode()
    assert L.sc_selfplay_traces_json(None, 0, None, None, 0, off.ctypes.data_as(C.c_void_p)) == -1
    assert L.sc_selfplay_write_traces_json(None, 0, None, None) == -1


def test_refuses_without_a_device(scamd):
    L = scamd.lib()
    if L.sc_device_count() > 0:
        pytest.skip("a GPU is present")
    off = np.zeros(1, np.uint64)
    assert L.sc_traces_format(0, 0, *[None] * 12, None, 0, off.ctypes.data_as(C.c_void_p)) == -3
    import scamd.traces as traces
    with pytest.raises(scamd.EngineError, match="no HIP device"):
        traces.format([{"steps": [], "outcome": None}])
