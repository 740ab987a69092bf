"""Shuffled training minibatches from the compact tensors, checks that need no GPU: sc_gather_batch is declared, bound and
exported; bad arguments are refused before anything touches a device; without a device every entry fails loudly; the replay
buffer's bookkeeping (ReplayIndex, numpy only) keeps whole games, evicts the oldest, follows the reference's start_step rule and
cuts an epoch as DataLoader(drop_last=True) does; and the numpy yardstick of the GPU tests (tests/batch_ref.py) is pinned on a
hand-written case."""
import os
import re
import subprocess

import numpy as np
import pytest

import batch_ref
from support import ROOT, _p, scamd_built  # noqa: F401


def _host_args():
    rows, mir = np.zeros(1, np.int32), np.zeros(1, np.uint8)
    b, m = np.zeros((1, 8, 8, 112), np.int8), np.zeros((1, 7), np.int32)
    dl, li, nl, oc = np.zeros((1, 224), np.float32), np.zeros((1, 224), np.uint16), np.zeros(1, np.int32), np.zeros(1, np.float32)
    return [rows, mir, b, m, dl, li, nl, oc]


def test_symbol_is_declared_bound_and_exported(scamd):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sc_engine.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", scamd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TW"}
    m = re.search(r"\bsc_gather_batch\s*\((.*?)\)\s*;", hdr, flags=re.S)
    assert m
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 17
    assert len(scamd.binding.ABI["sc_gather_batch"][1]) == 17
    assert "sc_gather_batch" in exported
    assert callable(scamd.gather_batch_torch) and callable(scamd.ReplayBuffer) and callable(scamd.ReplayIndex)
    assert scamd.binding.PLY_BYTES == 8548


def test_bad_arguments_are_refused_before_the_device(scamd):
    L = scamd.lib()
    a = _host_args()
    out = np.zeros(7168, np.float32)
    call = lambda n_src, n_batch, args: L.sc_gather_batch(0, n_src, n_batch, *[None if x is None else _p(x) for x in args], None, _p(out),
                                                          None, None, None, None)
    assert call(-1, 1, a) == -1 and "bad argument" in L.sc_last_error().decode()
    assert call(1, -1, a) == -1
    for k in (0, 2, 3, 4, 5, 6, 7):   # every source but mirror is needed
        assert call(1, 1, a[:k] + [None] + a[k + 1:]) == -1, k


def test_fails_loudly_without_gpu(scamd):
    L = scamd.lib()
    if L.sc_device_count() > 0:
        pytest.skip("a GPU is present")
    a = _host_args()
    out = np.zeros(7168, np.float32)
    rc = L.sc_gather_batch(0, 1, 1, *[_p(x) for x in a], None, _p(out), None, None, None, None)
    assert rc == -3 and "no HIP device" in L.sc_last_error().decode()
    with pytest.raises(scamd.EngineError, match="no HIP device"):
        scamd.gather_batch_torch({}, None)
    rb = scamd.ReplayBuffer(100)   # (nothing is allocated before the first use)
    with pytest.raises(scamd.EngineError, match="no HIP device"):
        rb.batches(8)
    with pytest.raises(scamd.EngineError, match="no HIP device"):
        rb.add({})


# ------------------------------------------------------------------ the bookkeeping
def _rows_of(ix, g):
    first, n = ix.games[g]
    return [(first + i) % ix.capacity for i in range(n)]


def test_index_evicts_the_oldest_whole_games(scamd):
    ix = scamd.ReplayIndex(20)
    assert ix.add_games([5, 6, 4]) == [(0, 0, 5), (5, 5, 6), (11, 11, 4)]
    assert ix.games == [(0, 5), (5, 6), (11, 4)] and ix.used == 15
    assert ix.eligible_rows().tolist() == list(range(15))
    # 7 more plies: 5 are free, the oldest game (5 plies) leaves -- whole -- and the new game wraps around the end
    assert ix.add_games([7]) == [(0, 15, 5), (5, 0, 2)]
    assert ix.games == [(5, 6), (11, 4), (15, 7)] and ix.used == 17
    assert ix.eligible_rows().tolist() == list(range(5, 15)) + [15, 16, 17, 18, 19, 0, 1]
    # 12 more: the two oldest leave (3 + 6 < 12 <= 3 + 6 + 4); no row of a kept game is overwritten
    copies = ix.add_games([12])
    assert ix.games == [(15, 7), (2, 12)] and copies == [(0, 2, 12)]
    kept, new = set(_rows_of(ix, 0)), set(_rows_of(ix, 1))
    assert not kept & new and len(kept | new) == ix.used == 19
    # a call whose games do not fit together: the first of them leaves again, the copies stay in order
    ix = scamd.ReplayIndex(10)
    copies = ix.add_games([6, 6])
    assert ix.games == [(6, 6)] and copies == [(0, 0, 6), (6, 6, 4), (10, 0, 2)]
    v = ix.version
    ix.add_games([1])
    assert ix.version != v


def test_index_start_step_is_the_reference_rule(scamd):
    """py/dataset.py:78-80: `if len(steps) < start_step: start_step = 0`, then steps[start_step:]"""
    ix = scamd.ReplayIndex(100, start_step=4)
    ix.add_games([3, 4, 9])   # shorter: all 3 plies; exactly start_step: none; longer: plies 4..8
    assert ix.eligible_rows().tolist() == [0, 1, 2] + list(range(3 + 4 + 4, 3 + 4 + 9))
    assert scamd.ReplayIndex(100).add_games([2]) == [(0, 0, 2)]
    ix0 = scamd.ReplayIndex(100, start_step=0)
    ix0.add_games([3, 0, 2])
    assert ix0.eligible_rows().tolist() == [0, 1, 2, 3, 4] and ix0.games == [(0, 3), (3, 2)]


def test_index_skips_failed_games_and_refuses_an_oversize_one(scamd):
    ix = scamd.ReplayIndex(10)
    assert ix.add_games([3, 4, 2], [0, 1002, 0]) == [(0, 0, 3), (7, 3, 2)]   # the source rows of the failed game are stepped over
    assert ix.games == [(0, 3), (3, 2)]
    assert ix.add_games([11], [-1]) == []   # a failed game is not looked at
    before = (list(ix.games), ix.head, ix.used)
    with pytest.raises(ValueError, match="11 plies"):
        ix.add_games([2, 11])
    assert (ix.games, ix.head, ix.used) == before   # refused before anything changed
    with pytest.raises(ValueError):
        ix.add_games([1, 2], [0])


def test_epoch_plan_is_drop_last(scamd):
    plan = scamd.ReplayIndex.epoch_plan
    for E, B in ((100, 8), (96, 8), (7, 8), (0, 8), (1024, 1024), (2047, 1024)):
        p = plan(E, B)
        assert len(p) == E // B and all(hi - lo == B for lo, hi in p)
        assert [lo for lo, _ in p] == [i * B for i in range(E // B)]
        q = plan(E, B, drop_last=False)
        assert len(q) == -(-E // B) and (not q or q[-1][1] == E)
    with pytest.raises(ValueError):
        plan(10, 0)
    seeds = {scamd.ReplayIndex.epoch_seed(s, e) for s in range(4) for e in range(4)}
    assert len(seeds) == 16 and all(0 <= x < 1 << 63 for x in seeds)
    assert scamd.ReplayIndex.epoch_seed(3, 1) == scamd.ReplayIndex.epoch_seed(3, 1)


# ------------------------------------------------------------------ the yardstick
def _hand_case():
    """two source rows.  Row 0: three legal moves -- action 0 with share 0.25, 17 with 0.5, 4671 with 0.25 -- and padding that
    points at action 0 with share 0 (as the encoder leaves it).  Row 1: Black to move, no legal move."""
    b = np.zeros((2, 8, 8, 112), np.int8)
    b[0, 1, 2, 3] = -128    # rank index 1, file index 2, plane 3
    b[0, 7, 7, 111] = 127
    b[1, 0, 0, 0] = -1
    m = np.array([[1, 12, 1, 0, 0, 1, 7], [0, 30, 0, 1, 1, 0, 99]], np.int32)
    li = np.zeros((2, 224), np.uint16)
    dl = np.zeros((2, 224), np.float32)
    li[0, :3] = [0, 17, 4671]
    dl[0, :3] = [0.25, 0.5, 0.25]
    return dict(boards=b, meta=m, legal_idx=li, dist_legal=dl, n_legal=np.array([3, 0], np.int32), outcome=np.array([1.0, 0.0], np.float32))


def test_yardstick_on_a_hand_written_case():
    src = _hand_case()
    ob, om, od, oo, n_bad = batch_ref.gather(src, [0, 1, 0], np.array([0, 1, 1], np.uint8))
    assert n_bad == 0
    # planes first, signed
    assert ob.shape == (3, 112, 8, 8) and ob[0, 3, 1, 2] == -128.0 and ob[0, 111, 7, 7] == 127.0 and ob[1, 0, 0, 0] == -1.0
    assert np.count_nonzero(ob[0]) == 2 and np.array_equal(ob[0], ob[2])   # the mirror leaves the planes alone
    # meta: plain; Black to move mirrored (fullmove stays); White to move mirrored (fullmove + 1); castling rights exchanged
    assert om[0].tolist() == [1, 12, 1, 0, 0, 1, 7]
    assert om[1].tolist() == [1, 30, 1, 0, 0, 1, 99]
    assert om[2].tolist() == [0, 13, 0, 1, 1, 0, 7]
    # dist: action 0 is a legal move and keeps its share
    exp = np.zeros(4672, np.float32)
    exp[[0, 17, 4671]] = [0.25, 0.5, 0.25]
    assert np.array_equal(od[0], exp) and np.array_equal(od[2], exp) and not od[1].any()
    # ... which scatter_add_ over the whole padded row gives too, and a plain scatter_ does not: a later padding entry
    # (action 0, share 0) overwrites action 0's share
    full_add = np.zeros(4672, np.float32)
    np.add.at(full_add, src["legal_idx"][0].astype(np.int64), src["dist_legal"][0])
    plain = np.zeros(4672, np.float32)
    for i in range(224):   # scatter_ in index order
        plain[src["legal_idx"][0, i]] = src["dist_legal"][0, i]
    assert np.array_equal(full_add, exp) and plain[0] == 0.0 and not np.array_equal(plain, exp)
    # outcome: negated under the mirror, -0.0 included (numpy's and the reference's float negation)
    assert oo.tolist() == [1.0, 0.0, -1.0] and np.signbit(oo[1]) and oo.dtype == np.float32
    # the same through torch's formulation of the dense row
    torch = pytest.importorskip("torch")
    t = torch.zeros(2, 4672).scatter_add_(1, torch.from_numpy(src["legal_idx"].astype(np.int64)), torch.from_numpy(src["dist_legal"]))
    assert np.array_equal(t.numpy()[0], od[0])


def test_yardstick_marks_bad_input():
    src = _hand_case()
    src["n_legal"] = np.array([219, 2], np.int32)
    src["legal_idx"][1, :2] = [5, 4672]
    ob, om, od, oo, n_bad = batch_ref.gather(src, [0, 1, -1, 2])
    assert n_bad == 4 and np.isnan(od).all()
    assert not np.isnan(ob[:2]).any() and not np.isnan(om[:2]).any() and not np.isnan(oo[:2]).any()
    assert np.isnan(ob[2:]).all() and np.isnan(om[2:]).all() and np.isnan(oo[2:]).all()
    src["n_legal"][1] = 1   # the bad index is padding now: not looked at
    assert batch_ref.gather(src, [1])[4] == 0
