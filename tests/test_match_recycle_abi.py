"""Match play with slot recycling, the checks that need no GPU: sc_selfplay_set_match / sc_selfplay_match_tally are exported with the
header's signatures, bound by scamd and by integration/hip.rs, and refuse to work without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from support import ROOT, scamd_built  # noqa: F401

NEW = {"sc_selfplay_set_match": ["sc_selfplay*", "sc_engine*", "sc_engine*", "uint64_t", "uint64_t", "int"],
       "sc_selfplay_match_tally": ["sc_selfplay*", "int64_t"]}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sc_engine.h")).read(), flags=re.S)


def _type(arg):
    """the type of a C parameter as the header spells it: its name and array brackets dropped"""
    arg = re.sub(r"\[\d*\]$", "", arg.strip())
    m = re.match(r"(.*?[\s*])([A-Za-z_]\w*)$", arg)
    return (m.group(1) if m else arg).strip()


def test_symbols_header_and_bindings_agree(scamd):
    hdr = _header()
    L = scamd.lib()
    rs = open(os.path.join(ROOT, "integration", "hip.rs")).read()
    ext = re.sub(r"//.*", "", re.search(r'extern "C" \{(.*?)\n\}', rs, flags=re.S).group(1))
    for name, want in NEW.items():
        m = re.search(rf"\bint\s+{name}\s*\((.*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        got = [_type(a) for a in m.group(1).split(",")]
        assert got == want, (name, got)
        assert hasattr(L, name), name
        res, args = scamd.binding.ABI[name]
        assert res is C.c_int and len(args) == len(want), name
        r = re.search(rf"fn {name}\((.*?)\)\s*->\s*c_int", ext, flags=re.S)
        assert r and len([a for a in r.group(1).split(",") if a.strip()]) == len(want), name
    assert scamd.binding.ABI["sc_selfplay_set_match"][1] == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int]
    assert callable(scamd.SelfPlay.set_match) and callable(scamd.SelfPlay.match_tally)
    # the lockstep entry point and its comment are what they were
    assert "Needs n_games == n_slots (all games advance in lockstep, no slot recycling)" in open(os.path.join(ROOT, "include", "sc_engine.h")).read()


def test_fails_loudly_without_gpu(scamd):
    L = scamd.lib()
    if L.sc_device_count() > 0:
        pytest.skip("a GPU is present")
    rc = L.sc_selfplay_set_match(None, None, None, 0x1111, 0x2222, 1)
    assert rc == -3 and "no HIP device" in L.sc_last_error().decode()
    out = np.zeros(8, np.int64)
    rc = L.sc_selfplay_match_tally(None, out.ctypes.data_as(C.c_void_p))
    assert rc == -3 and "no HIP device" in L.sc_last_error().decode()
    with pytest.raises(scamd.EngineError, match="no HIP device"):
        scamd.SelfPlay(None, n_slots=2, n_games=6, evaluator="synth").set_match(None, None, 1, 2)
