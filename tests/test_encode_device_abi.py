"""Device-resident training tensors, checks that need no GPU: the two entry points are declared, bound and exported, they
refuse loudly without a device, and the dist_legal -> dense rebuild the header documents (scatter_add_, not scatter_) is
right even where action 0 is a legal move."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from support import ROOT, scamd_built  # noqa: F401

NEW = ("sc_encode_steps_device", "sc_selfplay_encode_traces")


def test_new_symbols_are_declared_bound_and_exported(scamd):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sc_engine.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", scamd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TW"}
    for name in NEW:
        m = re.search(rf"\b{name}\s*\((.*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert len(scamd.binding.ABI[name][1]) == n_args, name
        assert name in exported, name
    assert len(scamd.binding.ABI["sc_encode_steps_device"][1]) == 18
    assert len(scamd.binding.ABI["sc_selfplay_encode_traces"][1]) == 14


def _runtimes_after(code):
    """libamdhip64 files mapped in a fresh interpreter after `code` (a fresh process: the order of the imports matters)"""
    import json
    import sys
    pre = "import sys, json; sys.path.insert(0, %r); " % os.path.join(ROOT, "smart-chess-rust_amd")
    r = subprocess.run([sys.executable, "-c", pre + code + "; import scamd; print(json.dumps(scamd.hip_runtime_files()))"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_hip_runtime_count_depends_on_import_order(scamd):
    """the premise of the torch functions' check: torch imported first -> libsc_engine.so binds to torch's runtime (one file
    mapped); scamd's library loaded first -> torch maps a second runtime, which hip_runtime_files() sees"""
    one = _runtimes_after("import scamd; scamd.lib()")
    assert len(one) == 1 and "libamdhip64" in os.path.basename(one[0]), one
    pytest.importorskip("torch")
    assert len(_runtimes_after("import torch; import scamd; scamd.lib()")) == 1
    assert len(_runtimes_after("import scamd; scamd.lib(); import torch")) == 2


def test_pack_steps_matches_the_list_form(scamd):
    games = [[("e2e4", [("e2e4", 3), ("d2d4", 1)]), ("e7e5", [("e7e5", 2)])], [], [("g1f3", [])]]
    mv, off, cm, cn, coff = scamd.pack_steps(games)
    assert off.tolist() == [0, 2, 2, 3] and coff.tolist() == [0, 2, 3, 3]
    assert mv.tolist() == [scamd.uci_move(u) for u in ("e2e4", "e7e5", "g1f3")]
    assert cm.tolist() == [scamd.uci_move(u) for u in ("e2e4", "d2d4", "e7e5")] and cn.tolist() == [3, 1, 2]
    assert mv.dtype == np.uint16 and off.dtype == np.uint32 and cn.dtype == np.uint32


def test_fails_loudly_without_gpu(scamd):
    L = scamd.lib()
    if L.sc_device_count() > 0:
        pytest.skip("a GPU is present")
    games = [[("e2e4", [("e2e4", 1)])]]
    with pytest.raises(scamd.EngineError, match="no HIP device"):
        scamd.encode_steps_torch(games)
    mv, off, cm, cn, coff = scamd.pack_steps(games)
    status = np.zeros(1, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = L.sc_encode_steps_device(None, 0, 1, p(mv), p(off), p(cm), p(cn), p(coff), 0, 1, None, None, None, None, None, None,
                                  None, p(status))
    assert rc == -3 and "no HIP device" in L.sc_last_error().decode()


def _rebuild_add(legal_idx, dist_legal):
    """numpy model of zeros(P, 4672).scatter_add_(1, legal_idx.long(), dist_legal)"""
    out = np.zeros((legal_idx.shape[0], 4672), np.float32)
    rows = np.repeat(np.arange(legal_idx.shape[0]), legal_idx.shape[1])
    np.add.at(out, (rows, legal_idx.reshape(-1).astype(np.int64)), dist_legal.reshape(-1))
    return out


def _rebuild_scatter(legal_idx, dist_legal):
    """numpy model of scatter_: for duplicate indices the last write wins (torch leaves the order unspecified)"""
    out = np.zeros((legal_idx.shape[0], 4672), np.float32)
    for r in range(legal_idx.shape[0]):
        for i in range(legal_idx.shape[1]):
            out[r, legal_idx[r, i]] = dist_legal[r, i]
    return out


def test_dist_legal_rebuild_needs_scatter_add(scamd):
    """a position where action 0 (a1 -> a2, one square north) is legal: White rook on a1, the a-pawn gone.  Padding entries
    (index 0, value 0) after n_legal would overwrite action 0's share with scatter_; scatter_add_ adds 0 to it."""
    assert scamd.encode_move(True, "a1a2") == 0
    legal = ["a1a2", "a1a3", "b1c3", "e2e4", "g1f3"]
    counts = np.array([7, 1, 0, 12, 3], np.uint32)
    den = np.float32(float(counts.sum()) + 1e-5)   # (float)sum + 1e-5f, as the kernel
    idx = np.zeros((2, 224), np.uint16)
    dl = np.zeros((2, 224), np.float32)
    ref = np.zeros((2, 4672), np.float32)
    for r in range(2):
        for i, u in enumerate(legal):
            idx[r, i] = scamd.encode_move(True, u)
            dl[r, i] = np.float32(counts[i]) / den
            ref[r, idx[r, i]] = dl[r, i]
    assert idx[0, 0] == 0 and ref[0, 0] > 0
    dense = _rebuild_add(idx, dl)
    assert np.array_equal(dense.view(np.uint32), ref.view(np.uint32))
    wrong = _rebuild_scatter(idx, dl)
    assert wrong[0, 0] == 0.0 and not np.array_equal(wrong, ref)
