"""C-ABI checks that need no GPU: libsc_engine.so loads, exports every symbol include/sc_engine.h declares,
refuses to compute without a device (no CPU fallback), and writes the reference's trace-file format."""
import ctypes as C
import json
import os
import re

import pytest
from support import GOLD, ROOT, scamd_built  # noqa: F401


def test_exports_exactly_the_declared_symbols(scamd):
    """header <-> library <-> binding: every declared entry point is exported, and nothing is exported that the header
    does not declare (no hidden developer entry points)"""
    import subprocess
    hdr = open(os.path.join(ROOT, "include", "sc_engine.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(sc_[a-z_0-9]+)\s*\(", hdr))
    assert len(declared) >= 30
    L = C.CDLL(scamd.lib_path())
    for name in declared:
        assert hasattr(L, name), name
    assert declared == set(scamd.binding.ABI), declared ^ set(scamd.binding.ABI)
    nm = subprocess.run(["nm", "-D", "--defined-only", scamd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TW" and ln.split()[-1].startswith("sc_")}
    assert exported == declared, exported ^ declared


def test_runtime_flags_report_the_kernarg_switch(scamd):
    """the load hook's effect on the process environment is queryable, and can be switched off (sc_engine.h)"""
    import subprocess
    import sys
    # (os.environ is a snapshot taken at interpreter start: ask the C library for the live value)
    code = ("import ctypes; L = ctypes.CDLL(%r); g = ctypes.CDLL(None).getenv; g.restype = ctypes.c_char_p; "
            "v = g(b'HIP_FORCE_DEV_KERNARG'); print(L.sc_runtime_flags(), v.decode() if v else None)" % scamd.lib_path())

    def run(env_extra, drop=()):
        env = {k: v for k, v in os.environ.items() if k not in ("HIP_FORCE_DEV_KERNARG", "SC_ENGINE_KEEP_ENV") + tuple(drop)}
        env.update(env_extra)
        # (the library is loaded directly: the ctypes binding sets the variable itself first -- it owns its process)
        return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, check=True).stdout.split()

    assert run({}) == ["3", "1"]                                  # set by the load hook: bits 0 + 1
    assert run({"HIP_FORCE_DEV_KERNARG": "1"}) == ["1", "1"]      # set by the host: effective for sure
    assert run({"HIP_FORCE_DEV_KERNARG": "0"}) == ["0", "0"]      # an explicit setting of the host wins
    assert run({"SC_ENGINE_KEEP_ENV": "1"}) == ["4", "None"]      # hook disabled: the environment is left alone


def test_product_does_not_reference_the_oracle():
    """the product path must never route through oracle/ (test infrastructure only)"""
    pkg = os.path.join(ROOT, "smart-chess-rust_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hpp", ".hip", ".cpp", ".h")):
                txt = open(os.path.join(d, f), errors="ignore").read()
                assert "oracle_py" not in txt and "sc_oracle" not in txt and "libsc_oracle" not in txt, f


def test_fails_loudly_without_gpu(scamd):
    if scamd.lib().sc_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(scamd.EngineError, match="no HIP device"):
        scamd.Engine(1, 256)
    with pytest.raises(scamd.EngineError, match="no HIP device"):
        scamd.SelfPlay(None, n_slots=2, evaluator="synth")
    with pytest.raises(scamd.EngineError, match="no HIP device"):
        scamd.encode_positions([[]])


def test_trace_json_format(scamd, tmp_path):
    fx = json.load(open(os.path.join(GOLD, "ref_fixtures.json")))
    # rebuild the reference-produced excerpt (older 3-field children) in today's 4-field shape
    steps = [(s[0], float(s[1]), [(c[0], c[1], float(c[2]), 0.5) for c in s[2]]) for s in fx["trace_first10"]]
    tr = {"steps": steps, "outcome": fx["trace_outcome"]}
    p = str(tmp_path / "trace.json")
    scamd.write_trace_json(p, tr)
    txt = open(p).read()
    back = json.load(open(p))
    assert list(back.keys()) == ["outcome", "steps"]                     # BTreeMap key order (src/trace.rs:24-27)
    assert back["outcome"] == {"termination": "Checkmate", "winner": "White"}
    assert [s[0] for s in back["steps"]] == [s[0] for s in steps]
    assert txt.startswith('{\n  "outcome": {\n    "termination": "Checkmate",\n    "winner": "White"\n  },\n  "steps": [\n    [\n      "g2g3",\n      11.045379638671875,\n      [\n        [\n          "g1h3",\n          23,\n          4.428466796875,\n          0.5\n        ],')
    # every float of the reference excerpt is reproduced digit for digit (f32 -> f64 -> shortest repr)
    for tok in re.findall(r"-?\d+\.\d+(?:e-?\d+)?", fx["trace_first10_text"]):
        assert re.search(r"(?<![\d.])" + re.escape(tok) + r"(?![\d])", txt), tok
    for s, b in zip(steps, back["steps"]):
        assert b[1] == s[1] and [tuple(c) for c in b[2]] == [tuple(c) for c in s[2]]
    # outcome null + empty children + exponent formats
    scamd.write_trace_json(p, {"steps": [("e7e8q", 1e-7, []), ("a2a1n", -0.0, [("h2h1r", 0, 1e20, 123456.5)])], "outcome": None})
    txt = open(p).read()
    assert '"outcome": null' in txt and '"e7e8q",\n      1.0000000116860974e-7,\n      []' in txt
    assert "1.0000000200408773e20" in txt and "123456.5" in txt and "-0.0" in txt
    assert json.load(open(p))["steps"][1][2][0][0] == "h2h1r"


def test_move_uci_roundtrip(scamd):
    for u in ["e2e4", "e1g1", "a7a8q", "h2h1n", "b7a8r", "c2d1b"]:
        assert scamd.move_uci(scamd.uci_move(u)) == u


def test_move_index_host_function(orc):
    """sc_move_index (libsmartchess.chess_encode_move) is a pure host function of the library: checked against the
    oracle on every legal move of random positions, and against the reference's recorded examples"""
    import scamd
    from helpers import random_games
    assert scamd.encode_move(True, "e2e4") == 877 and scamd.encode_move(True, "g1f3") == 501
    n = 0
    for moves, st in random_games(orc, 60, 80, seed=3):
        for m in st.legal_moves():
            assert scamd.encode_move(st.turn, m) == orc.move_index(m, st.turn)
            n += 1
    assert n > 1000


# ---------------------------------------------------------------------------------- struct layouts: header == Rust == ctypes
_RUST_T = {"i32": ("int32_t", C.c_int32), "u64": ("uint64_t", C.c_uint64), "i64": ("int64_t", C.c_int64), "f32": ("float", C.c_float)}
_STRUCTS = {"ScNetConfig": ("sc_net_config", "NetConfig"), "ScSelfplayConfig": ("sc_selfplay_config", "SelfplayConfig"),
            "ScSelfplayStats": ("sc_selfplay_stats", "Stats"), "ScTraceInfo": ("sc_trace_info", "TraceInfo")}


def _rust_structs(src):
    out = {}
    for name, body in re.findall(r"#\[repr\(C\)\]\s*pub struct (\w+)\s*\{(.*?)\}", src, flags=re.S):
        body = re.sub(r"//.*", "", body)
        out[name] = [(f, t) for f, t in re.findall(r"(?:pub\s+)?(\w+)\s*:\s*([\w\[\]; ]+?)\s*,", body)]
    return out


def _c_structs(hdr):
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = {}
    for body, name in re.findall(r"typedef struct\s*\{(.*?)\}\s*(\w+)\s*;", hdr, flags=re.S):
        out[name] = [(f, t) for t, f in re.findall(r"(\w+)\s+(\w+)\s*;", body)]
    return out


def test_rust_binding_structs_match_the_header(scamd):
    """integration/hip.rs (the reference-side binding, src/game.rs:3-21's implementor) declares every struct of the ABI with the
    header's fields -- same names, order and types -- and so does the ctypes binding; sizes and offsets agree with what a C
    compiler makes of the header (csrc/engine.hip pins those with static_asserts).  VERDICT r02: the documented Rust
    struct had fallen 8 bytes behind the header."""
    rs = _rust_structs(open(os.path.join(ROOT, "integration", "hip.rs")).read())
    cs = _c_structs(open(os.path.join(ROOT, "include", "sc_engine.h")).read())
    assert set(_STRUCTS.values()) and set(cs) == {v[0] for v in _STRUCTS.values()}, set(cs)
    for rname, (cname, pyname) in _STRUCTS.items():
        rfields, cfields = rs[rname], cs[cname]
        py = getattr(scamd.binding, pyname)
        assert [f for f, _ in rfields] == [f for f, _ in cfields] == [f for f, _ in py._fields_], rname
        for (f, rt), (_, ct), (_, pt) in zip(rfields, cfields, py._fields_):
            assert _RUST_T[rt][0] == ct and _RUST_T[rt][1] is pt, (rname, f, rt, ct, pt)
        # the C layout rules applied to the Rust field list (repr(C)) give the ctypes size and offsets
        off = 0
        for f, rt in rfields:
            sz = C.sizeof(_RUST_T[rt][1])
            off = (off + sz - 1) // sz * sz
            assert getattr(py, f).offset == off, (rname, f)
            off += sz
        align = max(C.sizeof(_RUST_T[rt][1]) for _, rt in rfields)
        assert C.sizeof(py) == (off + align - 1) // align * align, rname
    assert C.sizeof(scamd.binding.NetConfig) == 24 and C.sizeof(scamd.binding.SelfplayConfig) == 88
    assert C.sizeof(scamd.binding.Stats) == 32 and C.sizeof(scamd.binding.TraceInfo) == 32
    # ... and the engine's own static_asserts carry the same numbers
    eng = open(os.path.join(ROOT, "smart-chess-rust_amd", "csrc", "engine.hip")).read()
    for cname, size in (("sc_net_config", 24), ("sc_selfplay_config", 88), ("sc_selfplay_stats", 32), ("sc_trace_info", 32)):
        assert f"SC_LAYOUT({cname}, {size});" in eng
        for f, _ in cs[cname]:
            assert re.search(rf"SC_FIELD\({cname}, {f}, \d+\)", eng), (cname, f)


def test_rust_binding_functions_are_the_headers(scamd):
    """every `extern "C"` function integration/hip.rs binds is declared in the header with the same number of parameters"""
    src = open(os.path.join(ROOT, "integration", "hip.rs")).read()
    ext = re.search(r'extern "C" \{(.*?)\n\}', src, flags=re.S).group(1)
    ext = re.sub(r"//.*", "", ext)
    rust_fns = {n: len([a for a in args.split(",") if a.strip()]) for n, args in re.findall(r"fn (sc_\w+)\((.*?)\)", ext, flags=re.S)}
    assert {"sc_engine_create", "sc_predict_batch", "sc_predict_batch_argmax", "sc_encode_positions", "sc_selfplay_create"} <= set(rust_fns)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sc_engine.h")).read(), flags=re.S)
    for name, n_args in rust_fns.items():
        m = re.search(rf"\b{name}\s*\((.*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        cargs = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(cargs) == n_args == len(scamd.binding.ABI[name][1]), (name, len(cargs), n_args)
    # INTEGRATION.md points at the file instead of carrying a second copy of the structs
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "integration/hip.rs" in doc and "#[repr(C)]" not in doc


# the names `from .binding import (...)` of scamd/__init__.py listed before the package was split into modules
_PUBLIC = {"ChessHip", "Engine", "EngineError", "Play", "SelfPlay", "encode_move", "encode_positions", "encode_steps", "encode_steps_batch",
           "encode_steps_torch", "score_torch", "compare_torch", "gather_batch_torch", "ReplayBuffer", "ReplayIndex", "pack_steps", "hip_runtime",
           "hip_runtime_files", "choose_child", "enqueue_interleaved", "elo", "find_max", "lib", "lib_path", "play_match", "runtime_flags", "search",
           "move_uci", "uci_move", "write_trace_json", "TERMINATION"}
_BINDING = {"ABI", "lib", "lib_path", "NetConfig", "SelfplayConfig", "Stats", "TraceInfo", "EngineError", "ERR_HANDOFF", "MAX_MOVES", "TERMINATION",
            "EVALUATORS", "hip_runtime_files", "hip_runtime", "move_uci", "uci_move", "encode_move", "runtime_flags", "encode_steps_last_timing"}


def test_public_names(scamd):
    """scamd exports what it exported as one module, no more and no less: besides those names its namespace holds only its own
    submodules (Python binds an imported submodule to its package), `binding` among them; and scamd.binding keeps what bench.py,
    the tools and the tests read from it"""
    import types
    public = {n for n in vars(scamd) if not n.startswith("_")}
    modules = {n for n in public if isinstance(getattr(scamd, n), types.ModuleType)}
    assert public - modules == _PUBLIC, (public - modules) ^ _PUBLIC
    assert "binding" in modules and all(getattr(scamd, n).__name__ == f"scamd.{n}" for n in modules), modules
    assert not [n for n in sorted(_BINDING) if not hasattr(scamd.binding, n)]


def test_import_leaves_torch_out_and_sets_the_kernarg_default(scamd):
    """in a fresh process `import scamd; scamd.lib()` does not import torch (a host decides the order of the two HIP runtimes
    itself) and leaves HIP_FORCE_DEV_KERNARG=1 in os.environ"""
    import subprocess
    import sys
    code = ("import os, sys; sys.path.insert(0, %r); import scamd; scamd.lib(); "
            "print('torch' in sys.modules, os.environ.get('HIP_FORCE_DEV_KERNARG'))" % os.path.join(ROOT, "smart-chess-rust_amd"))
    env = {k: v for k, v in os.environ.items() if k != "HIP_FORCE_DEV_KERNARG"}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, check=True)
    assert r.stdout.split() == ["False", "1"], r.stdout + r.stderr
