"""CPU: the product tree and its one build recipe -- every source unit is in build.py's list (a second copy of that list, in a
script, once went stale and built libraries that did not load), nothing under smart-chess-rust_amd/ includes a file from outside
csrc/ and include/, and a variant build compiles the same units with the given defines and leaves lib/ alone."""
import os
import re
import sys

from support import ROOT

PKG = os.path.join(ROOT, "smart-chess-rust_amd")
CSRC = os.path.join(PKG, "csrc")
sys.path.insert(0, PKG)
import build as scbuild  # noqa: E402

# translation units that are not part of libsc_engine.so: the two command-line programs and the host build of the rules
OWN_TARGETS = {"selfplay_main.cpp", "play_main.cpp", "rules_host_api.cpp"}


def test_every_source_unit_is_in_the_unit_list():
    listed = [u for u, _ in scbuild.HIP_UNITS] + list(scbuild.CPP_UNITS)
    assert len(listed) == len(set(listed))
    on_disk = {f for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp"))}
    assert OWN_TARGETS <= on_disk
    assert set(listed) == on_disk - OWN_TARGETS


def test_no_include_leaves_the_product_tree():
    inside = set(os.listdir(CSRC)) | set(os.listdir(os.path.join(ROOT, "include")))
    seen = 0
    for d, _, files in os.walk(PKG):
        for f in files:
            if not f.endswith((".hpp", ".hip", ".cpp", ".h")):
                continue
            for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(d, f), errors="ignore").read(), re.M):
                seen += 1
                path = os.path.normpath(os.path.join(d, inc))
                assert os.path.dirname(path) in (CSRC, os.path.join(ROOT, "include")) and os.path.basename(path) in inside, (f, inc)
    assert seen > 50   # (the walk found the sources)


def test_variant_build_compiles_the_same_units_with_the_defines(tmp_path, monkeypatch):
    cmds = []
    monkeypatch.setattr(scbuild, "_run", lambda cmd: cmds.append(cmd) or "")
    lib = os.path.join(PKG, "lib")
    before = {f: os.stat(os.path.join(lib, f)).st_mtime_ns for f in os.listdir(lib)} if os.path.isdir(lib) else None
    out = str(tmp_path / "lib_variant")
    so = scbuild.build(out=out, defines=["SC_T8_RS=3", "SC_PROBE"])
    assert so == os.path.join(out, "libsc_engine.so")
    compiles = [c for c in cmds if "-c" in c]
    units = [os.path.basename(c[c.index("-c") + 1]) for c in compiles]
    assert units == [u for u, _ in scbuild.HIP_UNITS] + list(scbuild.CPP_UNITS)
    for c, (_, extra) in zip(compiles, scbuild.HIP_UNITS):
        assert all(x in c for x in extra) and "--offload-arch=gfx950" in c and "-O3" in c
    for c in compiles:
        assert "-DSC_T8_RS=3" in c and "-DSC_PROBE" in c
        assert c[c.index("-o") + 1].startswith(out + os.sep)
    (link,) = [c for c in cmds if "-c" not in c]
    assert "-shared" in link and link[link.index("-o") + 1] == so
    assert len([a for a in link if a.endswith(".o")]) == len(units)
    after = {f: os.stat(os.path.join(lib, f)).st_mtime_ns for f in os.listdir(lib)} if os.path.isdir(lib) else None
    assert before == after
