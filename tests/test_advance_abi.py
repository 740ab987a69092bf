"""CPU: sc_selfplay_advance is declared where every entry point is -- the header, the library's exports, the ctypes binding and
the reference-side Rust binding -- with one parameter list, and its units are built as the search's other units are."""
import ctypes as C
import os
import re
import subprocess

from support import ROOT, scamd_built  # noqa: F401

NAME = "sc_selfplay_advance"


def test_header_library_ctypes_and_rust_declare_it(scamd):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sc_engine.h")).read(), flags=re.S)
    m = re.search(rf"\bint\s+{NAME}\s*\((.*?)\)\s*;", hdr, flags=re.S)
    assert m, "the header declares it"
    cargs = [a.strip() for a in m.group(1).split(",")]
    assert cargs == ["sc_selfplay*", "int n", "const int32_t* slots", "const uint16_t* moves", "int32_t* status", "int32_t* kept"]
    nm = subprocess.run(["nm", "-D", "--defined-only", scamd.lib_path()], capture_output=True, text=True, check=True).stdout
    assert any(ln.split()[-1] == NAME and ln.split()[1] == "T" for ln in nm.splitlines() if len(ln.split()) == 3)
    res, args = scamd.binding.ABI[NAME]
    assert res is C.c_int and len(args) == len(cargs) and args[1] is C.c_int
    assert getattr(scamd.lib(), NAME).argtypes == args
    rs = open(os.path.join(ROOT, "integration", "hip.rs")).read()
    r = re.search(rf"fn {NAME}\((.*?)\)\s*->\s*c_int;", rs, flags=re.S)
    assert r and [a.split(":")[1].strip() for a in r.group(1).split(",")] == ["*mut ScSelfplay", "c_int", "*const i32", "*const u16", "*mut i32", "*mut i32"]


def test_refused_without_a_handle(scamd):
    assert scamd.lib().sc_selfplay_advance(None, 0, None, None, None, None) == -1
    assert b"bad argument" in scamd.lib().sc_last_error()


def test_units_are_built_like_the_other_search_units(scamd):
    import build as scbuild
    units = dict(scbuild.HIP_UNITS)
    assert units["advance_kernels.hip"] == units["mcts_kernels.hip"] == ["-ffp-contract=off"] and units["advance.hip"] == []
    src = open(os.path.join(ROOT, "smart-chess-rust_amd", "csrc", "advance_kernels.hip")).read()
    # the rules and the end of the ply are the search's own functions, not copies
    for fn in ("make_move", "rep_flags_wave", "outcome_claim_draw", "finish_game", "legal_has_move"):
        assert re.search(rf"\b{fn}\(", src) and not re.search(rf"^\s*(__device__|inline|static).*\b{fn}\s*\(", src, flags=re.M), fn
    assert '#include "search_expand.hpp"' in src
    assert hasattr(scamd.SelfPlay, "advance") and "keep_tree" in scamd.Play.__init__.__code__.co_varnames
