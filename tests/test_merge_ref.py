"""Merging identical training positions, checks that need no GPU: the numpy yardstick of the GPU tests (tests/merge_ref.py) pinned
on a hand-written case; sc_merge_positions and sc_merge_positions_workspace declared, bound and exported; bad arguments refused
before anything touches a device; without a device the call fails loudly."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import merge_ref
from support import ROOT, _p, scamd_built  # noqa: F401


def _hand_case():
    """5 rows.  0 and 2: equal samples (3 legal moves) with different shares, outcome and padding; 1: as 0 but for meta[6];
    3: as 0 but for the last legal index; 4: n_legal 219"""
    b = np.zeros((5, 8, 8, 112), np.int8)
    b[:, 1, 2, 3] = -128
    m = np.tile(np.array([1, 12, 1, 0, 0, 1, 7], np.int32), (5, 1))
    li = np.zeros((5, 224), np.uint16)
    li[:, :3] = [0, 17, 4671]
    dl = np.zeros((5, 224), np.float32)
    dl[:, :3] = [0.25, 0.5, 0.25]
    dl[2, :3] = [0.5, 0.0, 0.5]
    dl[0, 3:], li[0, 3:] = np.nan, 65535       # padding: not looked at
    dl[2, 3:], li[2, 3:] = 7.0, 9
    m[1, 6] = 8
    li[3, 2] = 4670
    nl = np.array([3, 3, 3, 3, 219], np.int32)
    oc = np.array([1.0, -1.0, 0.0, 1.0, -1.0], np.float32)
    return dict(boards=b, meta=m, legal_idx=li, dist_legal=dl, n_legal=nl, outcome=oc)


def test_yardstick_on_a_hand_written_case():
    src = _hand_case()
    out, group_of, counts = merge_ref.merge(src)
    assert group_of.tolist() == [0, 1, 0, 2, 3]
    assert counts.tolist() == [4, 1, 0, 2]
    assert out["count"].tolist() == [2, 1, 1, 1] and out["first"].tolist() == [0, 1, 3, 4]
    # the merged row: the head's input and padding bits, the mean shares and outcome
    assert out["dist_legal"][0, :3].tolist() == [0.375, 0.25, 0.375] and out["outcome"][0] == 0.5
    assert np.isnan(out["dist_legal"][0, 3:]).all() and (out["legal_idx"][0, 3:] == 65535).all()
    assert out["legal_idx"][0, :3].tolist() == [0, 17, 4671] and out["n_legal"][0] == 3
    # groups of one are their source rows, the bad one included, bit for bit
    for j, r in ((1, 1), (2, 3), (3, 4)):
        for k in merge_ref.KEYS:
            assert out[k][j].tobytes() == src[k][r].tobytes(), (j, k)
    assert out["n_legal"][3] == 219
    # rows: a subset with a repeat and two indices outside the source
    out, group_of, counts = merge_ref.merge(src, rows=[2, -1, 0, 2, 5, 4])
    assert group_of.tolist() == [0, -1, 0, 0, -1, 1] and counts.tolist() == [2, 3, 0, 3]
    assert out["first"].tolist() == [0, 5] and out["count"].tolist() == [3, 1]
    s = np.float32(np.float32(np.float32(0.5) + np.float32(0.25)) + np.float32(0.5))
    assert out["dist_legal"][0, 0] == np.float32(s / np.float32(3)) and out["dist_legal"][0, 3] == 7.0   # the head is source row 2
    assert merge_ref.mean_f32([np.float32(0.1)] * 3) == np.float32(np.float32(np.float32(0.1) + np.float32(0.1)) + np.float32(0.1)) / np.float32(3)


def test_generated_sources_are_what_the_gpu_tests_need():
    base = merge_ref.make_source()
    assert set(base["n_legal"].tolist()) == set(merge_ref.N_LEGAL)
    _, groups, n_bad = merge_ref.partition(base)
    assert len(groups) == 37 and n_bad == 0
    copies = [1 + (r * 7) % 11 for r in range(37)]
    copies[3], copies[10] = 65, 130
    src, origin = merge_ref.expand(base, copies)
    group_of, groups, _ = merge_ref.partition(src)
    assert sorted(len(g) for g in groups)[-2:] == [65, 130] and len(groups) == 37
    assert all(len({int(origin[p]) for p in g}) == 1 for g in groups)
    for r in range(len(origin)):
        n = int(src["n_legal"][r])
        sh = src["dist_legal"][r, :n]
        assert ((sh == 0) | ((sh >= 2.0 ** -20) & (sh <= 1))).all()
        assert np.isnan(src["dist_legal"][r, n:]).any() or n > 215
    assert (src["legal_idx"] > 4671).any() and set(np.unique(src["outcome"]).tolist()) == {-1.0, 0.0, 1.0}


def _declared(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sc_engine.h")).read(), flags=re.S)
    m = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, hdr, flags=re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_symbols_are_declared_bound_and_exported(scamd):
    """(24 parameters: the prototype's count)"""
    nm = subprocess.run(["nm", "-D", "--defined-only", scamd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TW"}
    for name, n_par in (("sc_merge_positions_workspace", 2), ("sc_merge_positions", 24)):
        assert _declared(name) == n_par, name
        assert len(scamd.binding.ABI[name][1]) == n_par, name
        assert name in exported, name
    assert callable(scamd.replay.merge_positions_torch) and callable(scamd.replay.unique_by_ply)
    assert callable(scamd.ReplayBuffer.merged)
    assert not hasattr(scamd, "merge_positions_torch")   # the submodule's, not the package's


def _host_args():
    return [np.zeros(1, np.int32), np.zeros((1, 8, 8, 112), np.int8), np.zeros((1, 7), np.int32), np.zeros((1, 224), np.float32),
            np.zeros((1, 224), np.uint16), np.zeros(1, np.int32), np.zeros(1, np.float32)]


def _call(L, n_src, n_in, args, key_bits=128, ws_bytes=None):
    need = C.c_size_t(0)
    assert L.sc_merge_positions_workspace(max(n_in, 0), C.byref(need)) == 0
    ws = np.zeros(need.value, np.uint8)
    counts = np.zeros(4, np.int32)
    return L.sc_merge_positions(0, n_src, n_in, *[None if x is None else _p(x) for x in args], key_bits, _p(ws),
                                need.value if ws_bytes is None else ws_bytes, None, *([None] * 9), _p(counts))


def test_workspace_size(scamd):
    L = scamd.lib()
    need = C.c_size_t(0)
    sizes = []
    for n in (0, 1, 400, 8192, 1 << 20):
        assert L.sc_merge_positions_workspace(n, C.byref(need)) == 0
        sizes.append(need.value)
    assert sizes == sorted(sizes) and sizes[0] > 0
    assert sizes[-1] < 200 * (1 << 20)   # a small share of the 8 548 bytes of a ply
    assert L.sc_merge_positions_workspace(-1, C.byref(need)) == -1 and "bad argument" in L.sc_last_error().decode()
    assert L.sc_merge_positions_workspace(1, None) == -1


def test_bad_arguments_are_refused_before_the_device(scamd):
    L = scamd.lib()
    a = _host_args()
    assert _call(L, -1, 1, a) == -1 and "bad argument" in L.sc_last_error().decode()
    assert _call(L, 1, -1, a) == -1
    assert _call(L, 1, 1, a, key_bits=129) == -1
    assert _call(L, 1, 1, a, key_bits=-1) == -1
    assert _call(L, 1, 2, [None] + a[1:]) == -1          # without rows n_in <= n_src
    assert _call(L, 1, 1, a, ws_bytes=64) == -1 and "workspace" in L.sc_last_error().decode()
    for k in range(1, 7):   # every source but rows is needed
        assert _call(L, 1, 1, a[:k] + [None] + a[k + 1:]) == -1, k


def test_fails_loudly_without_gpu(scamd):
    L = scamd.lib()
    if L.sc_device_count() > 0:
        pytest.skip("a GPU is present")
    assert _call(L, 1, 1, _host_args()) == -3 and "no HIP device" in L.sc_last_error().decode()
    with pytest.raises(scamd.EngineError, match="no HIP device"):
        scamd.replay.merge_positions_torch({})
    with pytest.raises(scamd.EngineError, match="no HIP device"):
        scamd.ReplayBuffer(100).merged()
