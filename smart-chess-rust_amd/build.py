"""Builds the in-tree native libraries (gfx950 only):

  lib/libsc_engine.so      HIP kernels + C ABI (include/sc_engine.h)          hipcc --offload-arch=gfx950
  lib/libsc_rules_host.so  host build of the device rules code for CPU tests   g++
  lib/sc-selfplay          CLI mirroring the reference's `selfplay` flags      g++
  lib/sc-play              CLI mirroring the reference's `play` flags (matches) g++

A variant of libsc_engine.so for same-box A/B runs (every unit, the production flags, extra defines) goes elsewhere:
  python build.py --out lib_ab --define SC_T8_AB=3
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "lib")
BUILD = os.path.join(HERE, "build")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _run(cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.stderr.write(" ".join(cmd) + "\n" + r.stdout + "\n")
        raise RuntimeError("build failed: " + " ".join(cmd[:4]))
    return r.stdout


# Every unit of libsc_engine.so, once: (HIP unit, its extra flags), and the plain C++ units (the SAN tokenizer and the FEN reader: no
# HIP in them, so that the same units also build into stand-alone programs).  tools/isa_compare.py reads the kernel units' pairs here.
HIP_UNITS = [
    ("mcts_kernels.hip", ["-ffp-contract=off"]), ("external_kernels.hip", ["-ffp-contract=off"]),
    ("advance_kernels.hip", ["-ffp-contract=off"]), ("encode_kernels.hip", ["-ffp-contract=off"]),
    ("nn_kernels.hip", ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]), ("step_kernels.hip", ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]),
    ("score_kernels.hip", ["-ffp-contract=off"]), ("report_kernels.hip", ["-ffp-contract=off"]),
    ("batch_kernels.hip", []), ("merge_kernels.hip", []), ("perft_kernels.hip", []), ("scan_kernels.hip", []), ("san_kernels.hip", []),
    ("san_write_kernels.hip", []), ("fen_kernels.hip", []), ("trace_kernels.hip", []), ("trace_write_kernels.hip", []),
    ("positions.hip", []), ("traces.hip", []), ("trace_write.hip", []), ("perft.hip", []), ("report.hip", []), ("advance.hip", []), ("engine.hip", []), ("encode_steps.hip", []),
    ("device_calls.hip", []), ("selfplay.hip", []), ("match_play.hip", []), ("external_play.hip", []), ("selfplay_io.hip", []),
    ("debug_calls.hip", []),
]
CPP_UNITS = ["san_tokens.cpp", "fen_text.cpp"]


def build(force=False, verbose=False, out=None, defines=()):
    """The default build: everything into lib/, units recompiled when stale.  With `out`: a variant of libsc_engine.so alone (same
    units, same flags, plus -D for every entry of `defines`) into that directory, objects under out/build; lib/ is not touched."""
    lib, objdir = (out, os.path.join(out, "build")) if out else (LIB, BUILD)
    force = force or bool(out)
    dflags = ["-D" + d for d in defines]
    os.makedirs(lib, exist_ok=True)
    os.makedirs(objdir, exist_ok=True)
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    hdrs.append(os.path.join(HERE, "..", "include", "sc_engine.h"))
    common = [HIPCC, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]
    objs = []
    for src, extra in HIP_UNITS:
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace(".hip", ".o"))
        if force or _newer(o, [s] + hdrs):
            text = _run(common + extra + dflags + ["-c", s, "-o", o])
            if verbose and text.strip():
                print(text)
        objs.append(o)
    for src in CPP_UNITS:
        s, o = os.path.join(CSRC, src), os.path.join(objdir, src.replace(".cpp", ".o"))
        if force or _newer(o, [s] + hdrs):
            _run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fPIC", "-fvisibility=hidden"] + dflags + ["-c", s, "-o", o])
        objs.append(o)
    so = os.path.join(lib, "libsc_engine.so")
    if force or _newer(so, objs):
        _run([HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", so] + objs + ["-Wl,-rpath,/opt/rocm/lib"])
    if out:
        return so
    host = os.path.join(LIB, "libsc_rules_host.so")
    hs = os.path.join(CSRC, "rules_host_api.cpp")
    if force or _newer(host, [hs] + hdrs):
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fPIC", "-shared", "-ffp-contract=off", "-o", host, hs])
    cli_src = os.path.join(CSRC, "selfplay_main.cpp")
    cli = os.path.join(LIB, "sc-selfplay")
    if os.path.exists(cli_src) and (force or _newer(cli, [cli_src, so] + hdrs)):
        _run(["g++", "-O2", "-std=c++17", "-pthread", cli_src, "-o", cli, "-L" + LIB, "-lsc_engine", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath-link,/opt/rocm/lib",
              "-Wl,-rpath,/opt/rocm/lib"])
    play_src = os.path.join(CSRC, "play_main.cpp")
    play = os.path.join(LIB, "sc-play")
    if os.path.exists(play_src) and (force or _newer(play, [play_src, so] + hdrs)):
        _run(["g++", "-O2", "-std=c++17", play_src, "-o", play, "-L" + LIB, "-lsc_engine", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath-link,/opt/rocm/lib",
              "-Wl,-rpath,/opt/rocm/lib"])
    return so


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="build the native libraries, or a variant of libsc_engine.so into another directory")
    ap.add_argument("--force", action="store_true", help="recompile every unit")
    ap.add_argument("--out", metavar="DIR", help="build libsc_engine.so alone into DIR (lib/ stays as it is)")
    ap.add_argument("--define", action="append", default=[], metavar="X[=v]", help="-D for every unit (with --out; repeatable)")
    a = ap.parse_args()
    if a.define and not a.out:
        ap.error("--define needs --out: the library in lib/ is the product")
    print(build(force=a.force, verbose=True, out=a.out, defines=a.define))
