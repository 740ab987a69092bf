"""Scoring networks on device tensors, on the GPU (-m gpu): sc_forward_device, sc_score_positions, sc_compare_engines.

Bit-exact where the same kernels or the same code run (forward against sc_forward_batch; one call against two calls over its
halves, a repeated call, the two dist forms' se / ent / value); against the float64 numpy yardstick of tests/score_ref.py on the
log-probabilities and values sc_forward_batch returns -- the entry point that exists without this feature -- within bounds
computed from the data: K = 14 roundings per term (the kernels' summation tree is 13 additions deep, score_kernels.hip) and
EPS_EXP = 2^-23 (expf: 1 ulp in HIP's math-function table).  Device buffers come from hipMalloc on the engine's HIP runtime; the
torch wrappers run in a child process."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import score_ref
from helpers import random_games, random_steps
from support import GOLD, ROOT, _p, dev_per_module, run_torch_child, scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu
GUARD = 0x5a5a5a5a


def _at(p, nbytes):
    return C.c_void_p(p.value + int(nbytes))


class Positions:
    """random games encoded by sc_encode_steps_device (layout 0): device pointers and host copies of everything"""

    def __init__(self, scamd, orc, dev, n_games, maxlen, seed, repeat=1):
        rnd = random.Random(seed)
        base = [g for g, _ in random_games(orc, n_games, maxlen, seed=seed) if g]
        # after 1. a4 the rook move a1-a2 is legal: action 0 (tests/test_encode_device_abi.py)
        base.append([orc.from_uci(u) for u in ("a2a4", "h7h6", "a1a3", "h6h5")])
        steps = [random_steps(orc, g, rnd, zero_share=0.2) for g in base * repeat]
        mv, off, cm, cn, coff = scamd.pack_steps(steps)
        n, P = len(steps), int(off[-1])
        self.P, self.dev = P, dev
        self.d = dict(boards=dev.alloc(P * 7168), meta=dev.alloc(P * 28), dist=dev.alloc(P * 4672 * 4), dist_legal=dev.alloc(P * 224 * 4),
                      legal_idx=dev.alloc(P * 448), n_legal=dev.alloc(P * 4))
        status = dev.alloc(n * 4)
        rc = scamd.lib().sc_encode_steps_device(None, 0, n, _p(mv), _p(off), _p(cm), _p(cn), _p(coff), 0, 0, dev.stream, self.d["boards"],
                                                self.d["meta"], self.d["dist"], self.d["dist_legal"], self.d["legal_idx"], self.d["n_legal"],
                                                status)
        assert rc == 0, scamd.lib().sc_last_error().decode()
        dev.sync()
        assert (dev.read(status, (n,), np.int32) == 0).all()
        self.boards = dev.read(self.d["boards"], (P, 8, 8, 112), np.int8)
        self.meta = dev.read(self.d["meta"], (P, 7), np.int32)
        self.dist = dev.read(self.d["dist"], (P, 4672), np.float32)
        self.dist_legal = dev.read(self.d["dist_legal"], (P, 224), np.float32)
        self.legal_idx = dev.read(self.d["legal_idx"], (P, 224), np.uint16)
        self.n_legal = dev.read(self.d["n_legal"], (P,), np.int32)
        win = np.asarray([rnd.choice((-1.0, 0.0, 1.0)) for _ in steps], np.float32)
        self.outcome = np.repeat(win, np.diff(off.astype(np.int64)))
        self.d["outcome"] = dev.upload(self.outcome)


@pytest.fixture(scope="module")
def big(scamd, orc, dev):
    """>= 20 000 plies (27 990 with these seeds): four slices of at most 8 192"""
    ps = Positions(scamd, orc, dev, 60, 150, seed=21, repeat=6)
    assert ps.P >= 20000
    return ps


def _forward_host(eng, ps, chunk=4096):
    """the yardstick's input: logp / value of sc_forward_batch"""
    lp = np.empty((ps.P, 4672), np.float32)
    v = np.empty(ps.P, np.float32)
    for a in range(0, ps.P, chunk):
        lp[a:a + chunk], v[a:a + chunk] = eng.forward(ps.boards[a:a + chunk], ps.meta[a:a + chunk])
    return lp, v


def _score(scamd, dev, eng, ps, form, a=0, n=None, outputs=True, stream=None):
    """sc_score_positions on positions [a, a + n) -> dict of host arrays; every output buffer has one guard entry past n"""
    n = ps.P - a if n is None else n
    d = ps.d
    out = {k: dev.alloc((n + 1) * 4) for k in ("ce", "se", "ent", "value")} if outputs else dict(ce=None, se=None, ent=None, value=None)
    summ = dev.alloc(6 * 8)
    dense = _at(d["dist"], a * 4672 * 4) if form == "dense" else None
    sp = (_at(d["dist_legal"], a * 896), _at(d["legal_idx"], a * 448), _at(d["n_legal"], a * 4)) if form == "sparse" else (None, None, None)
    rc = scamd.lib().sc_score_positions(eng.h, n, _at(d["boards"], a * 7168), _at(d["meta"], a * 28), dense, sp[0], sp[1], sp[2],
                                        _at(d["outcome"], a * 4), stream or dev.stream, out["ce"], out["se"], out["ent"], out["value"], summ)
    assert rc == 0, scamd.lib().sc_last_error().decode()
    dev.sync()
    r = {}
    for k, p in out.items():
        if p is not None:
            full = dev.read(p, (n + 1,), np.float32)
            assert full[n:].view(np.uint32)[0] == GUARD, k          # nothing beyond n entries is written
            r[k] = full[:n]
    s = dev.read(summ, (6,), np.float64)
    assert s[5:].view(np.uint64)[0] == 0x5a5a5a5a5a5a5a5a
    r["summary"] = s[:5]
    return r


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("prec,C", [("bf16", 128), ("fp8", 128), ("bf16", 256), ("fp8", 256)])
def test_forward_device_is_forward_batch_bit_for_bit(scamd, dev, big, prec, C):
    eng = scamd.Engine(2, C, seed=4, precision=prec)
    try:
        n = 333   # not a multiple of the 64-position tiles of value_head.ffn.0
        a = big.P // 2
        logp_h, val_h = eng.forward(big.boards[a:a + n], big.meta[a:a + n])
        d_logp, d_val = dev.alloc((n + 1) * 4672 * 4), dev.alloc((n + 1) * 4)
        L = scamd.lib()
        rc = L.sc_forward_device(eng.h, n, _at(big.d["boards"], a * 7168), _at(big.d["meta"], a * 28), dev.stream, d_logp, d_val)
        assert rc == 0, L.sc_last_error().decode()
        dev.sync()
        lp = dev.read(d_logp, (n + 1, 4672), np.float32)
        v = dev.read(d_val, (n + 1,), np.float32)
        assert np.array_equal(_bits(lp[:n]), _bits(logp_h)) and np.array_equal(_bits(v[:n]), _bits(val_h))
        assert (_bits(lp[n]) == GUARD).all() and _bits(v[n:])[0] == GUARD
        # without the log-probabilities; on the default stream
        d_val2 = dev.alloc((n + 1) * 4)
        assert L.sc_forward_device(eng.h, n, _at(big.d["boards"], a * 7168), _at(big.d["meta"], a * 28), None, None, d_val2) == 0
        assert eng.L.sc_engine_synchronize(eng.h) == 0   # (the engine's stream waits for the call)
        assert np.array_equal(_bits(dev.read(d_val2, (n,), np.float32)), _bits(val_h))
    finally:
        eng.close()


def test_forward_device_across_slices(scamd, dev, big):
    """all >= 20 000 positions in one call (three slices) = sc_forward_batch, values and log-probabilities"""
    eng = scamd.Engine(1, 128, seed=2)
    try:
        lp_h, v_h = _forward_host(eng, big)
        d_logp, d_val = dev.alloc(big.P * 4672 * 4), dev.alloc(big.P * 4)
        rc = scamd.lib().sc_forward_device(eng.h, big.P, big.d["boards"], big.d["meta"], dev.stream, d_logp, d_val)
        assert rc == 0, scamd.lib().sc_last_error().decode()
        dev.sync()
        assert np.array_equal(_bits(dev.read(d_val, (big.P,), np.float32)), _bits(v_h))
        assert np.array_equal(_bits(dev.read(d_logp, (big.P, 4672), np.float32)), _bits(lp_h))
    finally:
        eng.close()


def _check_against_yardstick(r, ref, form):
    for k, b in (("ce", "b_ce"), ("se", "b_se"), ("ent", "b_ent")):
        err = np.abs(r[k].astype(np.float64) - ref[k])
        worst = int(np.argmax(err - ref[b]))
        print(f"{form} {k}: max |err| {err.max():.3e}, at the position nearest its bound {err[worst]:.3e} of {ref[b][worst]:.3e}")
        assert (err <= ref[b]).all(), (k, worst, err[worst], ref[b][worst])


def _check_summary(r):
    s = r["summary"]
    assert s[0] == r["ce"].size and s[4] == 0
    for i, k in ((1, "ce"), (2, "se"), (3, "ent")):
        x = r[k].astype(np.float64)
        assert abs(s[i] - x.mean()) <= score_ref.mean_bound(x), (k, s[i], x.mean())


def test_score_positions_across_slices(scamd, dev, big):
    """>= 20 000 positions, both dist forms: the yardstick, the summary, halves, a repeated call, the guard entries"""
    nl = big.n_legal
    has0 = np.nonzero(((big.legal_idx == 0) & (np.arange(224)[None, :] < nl[:, None])).any(1))[0]
    assert has0.size > 0, "no position whose action 0 is legal: extend the set"
    widest = int(np.argmax(nl))
    eng = scamd.Engine(2, 128, seed=4)
    try:
        lp, v = _forward_host(eng, big)
        ref = score_ref.score(lp, v, big.dist, big.outcome)
        dense = _score(scamd, dev, eng, big, "dense")
        sparse = _score(scamd, dev, eng, big, "sparse")
        print(f"P = {big.P}, action 0 legal in {has0.size} positions, widest position {widest} with {int(nl[widest])} moves")
        assert np.array_equal(_bits(dense["value"]), _bits(v))
        _check_against_yardstick(dense, ref, "dense")
        _check_against_yardstick(sparse, ref, "sparse")
        for k in ("se", "ent", "value"):
            assert np.array_equal(_bits(dense[k]), _bits(sparse[k])), k
        gap = np.abs(dense["ce"].astype(np.float64) - sparse["ce"].astype(np.float64))
        assert (gap <= 2 * ref["b_ce"]).all()
        for p in (int(has0[0]), widest):
            assert abs(float(sparse["ce"][p]) - ref["ce"][p]) <= ref["b_ce"][p] and abs(float(dense["ce"][p]) - ref["ce"][p]) <= ref["b_ce"][p]
        _check_summary(dense)
        _check_summary(sparse)
        # a second identical call: every bit again, the summary included
        for form, first in (("dense", dense), ("sparse", sparse)):
            again = _score(scamd, dev, eng, big, form)
            for k in ("ce", "se", "ent", "value", "summary"):
                assert np.array_equal(_bits(first[k]), _bits(again[k])), (form, k)
        # two calls over the halves (the cut is no multiple of a slice, a tile or a workgroup)
        h = big.P // 2 + 1
        for form, whole in (("dense", dense), ("sparse", sparse)):
            lo, hi = _score(scamd, dev, eng, big, form, 0, h), _score(scamd, dev, eng, big, form, h, big.P - h)
            for k in ("ce", "se", "ent", "value"):
                assert np.array_equal(_bits(np.concatenate([lo[k], hi[k]])), _bits(whole[k])), (form, k)
        # per-position outputs not asked for: the summary is the same
        only = _score(scamd, dev, eng, big, "sparse", outputs=False)
        assert np.array_equal(_bits(only["summary"]), _bits(sparse["summary"]))
        # n = 0
        zero = _score(scamd, dev, eng, big, "dense", 0, 0)
        assert not zero["summary"].any()
    finally:
        eng.close()


def _compare(scamd, dev, ea, eb, d_boards, d_meta, n):
    tv, dv, summ = dev.alloc((n + 1) * 4), dev.alloc((n + 1) * 4), dev.alloc(10 * 8)
    rc = scamd.lib().sc_compare_engines(ea.h, eb.h, n, d_boards, d_meta, dev.stream, tv, dv, summ)
    assert rc == 0, scamd.lib().sc_last_error().decode()
    dev.sync()
    t, d, s = dev.read(tv, (n + 1,), np.float32), dev.read(dv, (n + 1,), np.float32), dev.read(summ, (10,), np.float64)
    assert _bits(t[n:])[0] == GUARD and _bits(d[n:])[0] == GUARD and _bits(s[9:])[0] == 0x5a5a5a5a5a5a5a5a
    return t[:n], d[:n], s[:9]


def _check_compare_summary(tv, dv, s):
    assert s[0] == tv.size
    for o, x in ((1, tv.astype(np.float64)), (5, dv.astype(np.float64))):
        assert abs(s[o] - x.mean()) <= score_ref.mean_bound(x)
        assert abs(s[o + 1] - x.std()) <= 1e-12 * max(x.std(), 1e-30) + 1e-15    # population standard deviation, two passes in double
        assert s[o + 2] == x.max() and s[o + 3] == x.min()


def test_compare_engines(scamd, dev, big):
    g = np.load(os.path.join(GOLD, "nn_ref_b10_c128.npz"))
    n = g["boards"].shape[0]
    d_b, d_m = dev.upload(g["boards"].astype(np.int8)), dev.upload(g["meta"].astype(np.int32))
    a = scamd.Engine(10, 128, seed=int(g["seed"]))
    b = scamd.Engine(10, 128, seed=int(g["seed"]), precision="fp8")
    a2 = scamd.Engine(10, 128, seed=int(g["seed"]))
    wide = scamd.Engine(1, 256, seed=3, precision="fp8")
    try:
        # an engine against itself, and against a second engine of the same weights: exactly 0
        for other in (a, a2):
            tv, dv, s = _compare(scamd, dev, a, other, d_b, d_m, n)
            assert not tv.any() and not dv.any() and s[0] == n and not s[1:].any()
        la, va = a.forward(g["boards"], g["meta"])
        lb, vb = b.forward(g["boards"], g["meta"])
        ref = score_ref.compare(la, va, lb, vb)
        tv, dv, s = _compare(scamd, dev, a, b, d_b, d_m, n)
        print(f"bf16 vs fp8, 10 x 128: tv max {tv.max():.4f} mean {tv.mean():.4f}; |err| max {np.abs(tv - ref['tv']).max():.3e} (bound {ref['b_tv'].max():.3e})")
        assert (np.abs(tv.astype(np.float64) - ref["tv"]) <= ref["b_tv"]).all() and tv.max() > 1e-4
        assert (np.abs(dv.astype(np.float64) - ref["dv"]) <= ref["b_dv"]).all()
        _check_compare_summary(tv, dv, s)
        # any pairing: depth, width and precision differ; across slices
        m = 8192 + 500
        lw, vw = wide.forward(big.boards[:m], big.meta[:m])
        l2, v2 = a.forward(big.boards[:m], big.meta[:m])
        ref = score_ref.compare(l2, v2, lw, vw)
        tv, dv, s = _compare(scamd, dev, a, wide, big.d["boards"], big.d["meta"], m)
        assert (np.abs(tv.astype(np.float64) - ref["tv"]) <= ref["b_tv"]).all()
        assert (np.abs(dv.astype(np.float64) - ref["dv"]) <= ref["b_dv"]).all()
        _check_compare_summary(tv, dv, s)
        tv2, dv2, s2 = _compare(scamd, dev, a, wide, big.d["boards"], big.d["meta"], m)
        assert np.array_equal(_bits(tv), _bits(tv2)) and np.array_equal(_bits(dv), _bits(dv2)) and np.array_equal(_bits(s), _bits(s2))
    finally:
        for e in (a, b, a2, wide):
            e.close()


def test_non_finite_rows_are_counted(scamd, dev, big, tmp_path):
    """a network with one NaN weight in the trunk: every row is NaN, every position is counted, the means are NaN, nothing faults;
    with the NaN in the value head only the policy figures stay finite"""
    import scw
    n = 100
    for key, pol_finite in (("res_blocks.0.conv1.bias", False), ("value_head.conv.0.bias", True)):
        sd = scw.prng_state_dict(2, 128, 7)
        sd[key] = sd[key].copy()
        sd[key][3] = np.nan
        path = str(tmp_path / "bad.scw")
        scw.write_scw(path, sd, 2, 128)
        bad = scamd.Engine(weights=path)
        good = scamd.Engine(2, 128, seed=7)
        try:
            r = _score(scamd, dev, bad, big, "sparse", 0, n)
            assert r["summary"][0] == n and r["summary"][4] == n
            assert np.isnan(r["se"]).all() and np.isnan(r["summary"][2])
            assert np.isfinite(r["ce"]).all() == pol_finite and np.isfinite(r["summary"][1]) == pol_finite
            assert np.isfinite(r["ent"]).all() == pol_finite and np.isfinite(r["summary"][3]) == pol_finite
            tv, dv, s = _compare(scamd, dev, good, bad, big.d["boards"], big.d["meta"], n)
            assert np.isnan(dv).all() and np.isnan(s[5:]).all()
            assert np.isfinite(tv).all() == pol_finite and np.isfinite(s[1:5]).all() == pol_finite
        finally:
            bad.close()
            good.close()


def test_refusals(scamd, dev, big):
    L = scamd.lib()
    eng = scamd.Engine(1, 128, seed=1)
    try:
        n = 8
        host_b = np.zeros((n, 8, 8, 112), np.int8)
        host_f = np.zeros(n, np.float32)
        out, summ = dev.alloc(n * 4), dev.alloc(9 * 8)
        d = big.d
        err = lambda: L.sc_last_error().decode()
        assert L.sc_forward_device(eng.h, n, _p(host_b), d["meta"], dev.stream, None, out) == -1 and "boards" in err() and "device memory" in err()
        assert L.sc_forward_device(eng.h, n, d["boards"], d["meta"], dev.stream, None, _p(host_f)) == -1 and "value" in err()
        assert L.sc_score_positions(eng.h, n, d["boards"], d["meta"], d["dist"], None, None, None, d["outcome"], dev.stream, _p(host_f), None,
                                    None, None, summ) == -1 and "ce" in err()
        assert L.sc_score_positions(eng.h, n, d["boards"], d["meta"], d["dist"], None, None, None, _p(host_f), dev.stream, out, None,
                                    None, None, summ) == -1 and "outcome" in err()
        assert L.sc_score_positions(eng.h, n, d["boards"], d["meta"], _at(d["dist"], 4), None, None, None, d["outcome"], dev.stream, out, None,
                                    None, None, summ) == -1 and "aligned" in err()
        assert L.sc_compare_engines(eng.h, eng.h, n, d["boards"], _p(np.zeros((n, 7), np.int32)), dev.stream, out, None, summ) == -1 and "meta" in err()
        if L.sc_device_count() > 1:
            other = scamd.Engine(1, 128, seed=1, device=1)
            try:
                assert L.sc_compare_engines(eng.h, other.h, n, d["boards"], d["meta"], dev.stream, out, None, summ) == -1 and "devices" in err()
                assert L.sc_forward_device(other.h, n, d["boards"], d["meta"], None, None, out) == -1 and "device" in err()
            finally:
                other.close()
        # n_legal > 218 and an action index past the row are found on the device: ce is NaN, the position is counted, its
        # neighbours are untouched (include/sc_engine.h)
        nl = big.n_legal[:n].copy()
        li = big.legal_idx[:n].copy()
        nl[2] = 219
        li[5, 0] = 4672
        nl[6] = -1
        d_nl, d_li = dev.upload(nl), dev.upload(li)
        ce, s5 = dev.alloc(n * 4), dev.alloc(5 * 8)
        rc = L.sc_score_positions(eng.h, n, d["boards"], d["meta"], None, d["dist_legal"], d_li, d_nl, d["outcome"], dev.stream, ce, None, None,
                                  None, s5)
        assert rc == 0, err()
        dev.sync()
        got = dev.read(ce, (n,), np.float32)
        clean = _score(scamd, dev, eng, big, "sparse", 0, n)
        assert np.isnan(got[[2, 5, 6]]).all() and dev.read(s5, (5,), np.float64)[4] == 3
        keep = [0, 1, 3, 4, 7]
        assert np.array_equal(_bits(got[keep]), _bits(clean["ce"][keep]))
        # ... and good calls still work after the refusals
        assert L.sc_forward_device(eng.h, n, d["boards"], d["meta"], dev.stream, None, out) == 0
        dev.sync()
    finally:
        eng.close()


_CHILD = r'''
import json, os, sys
import torch                      # first: libsc_engine.so then binds to the runtime torch loaded
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import numpy as np
import scamd
import score_ref
out = {}
torch.zeros(1, device="cuda:0")
eng = scamd.Engine(1, 128, seed=6)
sp = scamd.SelfPlay(eng, n_slots=64, n_games=64, rollout_num=16, num_steps=12, temperature=1.0, temperature_switch=6, seed=3,
                    outcome_gate=4)
sp.run()
fin = sp.poll()
out["finished"] = len(fin)
t = sp.training_tensors(sorted(fin), layout="reference", dist="legal")
P = t["boards"].shape[0]
out["P"] = P
r = scamd.score_torch(eng, t)
torch.cuda.synchronize()
b, m = t["boards"].cpu().numpy(), t["meta"].cpu().numpy()
logp, value = eng.forward(b, m)
dist = score_ref.dense_from_sparse(t["dist_legal"].cpu().numpy(), t["legal_idx"].cpu().numpy().view(np.uint16), t["n_legal"].cpu().numpy())
ref = score_ref.score(logp, value, dist, t["outcome"].cpu().numpy())
ce = r["ce"].cpu().numpy()
out["loss1"], out["loss2"], out["pi_entropy"], out["n_nonfinite"] = r["loss1"], r["loss2"], r["pi_entropy"], r["n_nonfinite"]
out["ce_in_bound"] = bool((np.abs(ce - ref["ce"]) <= ref["b_ce"]).all())
out["ent_in_bound"] = bool((np.abs(r["ent"].cpu().numpy() - ref["ent"]) <= ref["b_ent"]).all())
out["se_in_bound"] = bool((np.abs(r["se"].cpu().numpy() - ref["se"]) <= ref["b_se"]).all())
out["loss1_ref"] = float(ref["ce"].mean())
out["loss1_bound"] = float(ref["b_ce"].mean() + score_ref.mean_bound(ce))
out["value_equal"] = bool(np.array_equal(r["value"].cpu().numpy().view(np.uint32), value.view(np.uint32)))
# dense form through the wrapper: the same se / ent / value bits
t2 = sp.training_tensors(sorted(fin), layout="reference", dist="dense")
r2 = scamd.score_torch(eng, t2)
out["forms_equal"] = bool(all(torch.equal(r[k], r2[k]) for k in ("se", "ent", "value")))
lp_t, v_t = eng.forward_torch(t["boards"], t["meta"])
torch.cuda.synchronize()
out["forward_torch_equal"] = bool(np.array_equal(lp_t.cpu().numpy().view(np.uint32), logp.view(np.uint32))
                                  and np.array_equal(v_t.cpu().numpy().view(np.uint32), value.view(np.uint32)))
eng8 = scamd.Engine(1, 128, seed=6, precision="fp8")
c = scamd.compare_torch(eng, eng8, t)
l8, v8 = eng8.forward(b, m)
cref = score_ref.compare(logp, value, l8, v8)
out["tv_in_bound"] = bool((np.abs(c["tv"].cpu().numpy() - cref["tv"]) <= cref["b_tv"]).all())
out["tv_mean"], out["tv_mean_ref"] = c["tv_mean"], float(cref["tv"].mean())
same = scamd.compare_torch(eng, eng, t)
out["self_zero"] = bool(same["tv_max"] == 0.0 and same["dv_max"] == 0.0 and same["n"] == P)
try:
    scamd.score_torch(eng, sp.training_tensors(sorted(fin), layout="trainer", dist="legal"))
    out["trainer_refused"] = ""
except ValueError as e:
    out["trainer_refused"] = str(e)
sp.close()
eng.close()
eng8.close()
print(json.dumps(out))
'''


def test_selfplay_to_losses_in_a_fresh_process(scamd, tmp_path):
    """SelfPlay end to end with torch in the process: 64 short games of a 1-block network, poll, training_tensors(layout=
    "reference", dist="legal"), score_torch with the playing engine -> finite loss1 equal to the yardstick on the same tensors;
    forward_torch and compare_torch next to the host entry points; the trainer layout is refused by name"""
    import torch  # noqa: F401  (a missing torch is a failure here, not a reason to skip)
    out = run_torch_child(tmp_path, _CHILD, os.path.join(ROOT, "smart-chess-rust_amd"), os.path.join(ROOT, "tests"), timeout=900)
    print(out)
    assert out["finished"] == 64 and out["P"] > 64 and out["n_nonfinite"] == 0, out
    assert np.isfinite(out["loss1"]) and np.isfinite(out["loss2"]) and np.isfinite(out["pi_entropy"]), out
    assert out["ce_in_bound"] and out["ent_in_bound"] and out["se_in_bound"] and out["value_equal"], out
    assert abs(out["loss1"] - out["loss1_ref"]) <= out["loss1_bound"], out
    assert out["forms_equal"] and out["forward_torch_equal"] and out["tv_in_bound"] and out["self_zero"], out
    assert abs(out["tv_mean"] - out["tv_mean_ref"]) <= 1e-6, out
    assert 'layout="reference"' in out["trainer_refused"], out


def test_validate_model_tool_end_to_end(scamd, tmp_path):
    """tools/validate_model.py on two trace files the library wrote and one seeded 2 x 128 blob as bf16 and as fp8: the printed
    dictionaries equal the yardstick on sc_forward_batch's outputs for the same positions; a wrong block count is refused"""
    import ast
    import scw
    import validate_model
    sp = scamd.SelfPlay(None, n_slots=2, n_games=2, rollout_num=8, num_steps=10, evaluator="synth", temperature=1.0, temperature_switch=6,
                        seed=3, outcome_gate=4)
    sp.run()
    traces = [str(tmp_path / f"trace{g}.json") for g in range(2)]
    for g, path in enumerate(traces):
        sp.write_trace(g, path)
    sp.close()
    blob = str(tmp_path / "net.scw")
    scw.write_scw(blob, scw.prng_state_dict(2, 128, 7), 2, 128)
    tool = os.path.join(ROOT, "tools", "validate_model.py")
    r = subprocess.run([sys.executable, tool, "-t", traces[0], "-t", traces[1], "--model1", "2:" + blob, "--model2", blob, "--precision2", "fp8",
                        "--losses"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    printed = {}
    for ln in r.stdout.splitlines():
        head, sep, tail = ln.partition(": {")
        if sep:
            printed[head] = ast.literal_eval("{" + tail)
    assert set(printed) == {"policy difference", "value difference", "model1", "model2"}, r.stdout
    games, wins = zip(*(validate_model.load_trace(p) for p in traces))
    h = scamd.encode_steps_batch(list(games))
    assert (h["status"] == 0).all()
    a, b = scamd.Engine(weights=blob), scamd.Engine(weights=blob, precision="fp8")
    try:
        la, va = a.forward(h["boards"], h["meta"])
        lb, vb = b.forward(h["boards"], h["meta"])
    finally:
        a.close()
        b.close()
    ref = score_ref.compare(la, va, lb, vb)
    for name, x, bound in (("policy difference", ref["tv"], ref["b_tv"]), ("value difference", ref["dv"], ref["b_dv"])):
        got = printed[name]
        assert list(got) == ["mean", "std", "max", "min"]
        tol = float(bound.max()) + 1e-12
        assert abs(got["mean"] - x.mean()) <= tol and abs(got["std"] - x.std()) <= 2 * tol, (name, got, x.mean(), x.std())
        assert abs(got["max"] - x.max()) <= tol and abs(got["min"] - x.min()) <= tol, (name, got)
    assert printed["policy difference"]["max"] > 1e-4
    oc = np.repeat(np.asarray(wins, np.float32), np.diff(h["ply_off"].astype(np.int64)))
    for name, lp, v in (("model1", la, va), ("model2", lb, vb)):
        s = score_ref.score(lp, v, h["dist"], oc)
        assert printed[name]["non_finite"] == 0
        assert abs(printed[name]["val_loss1"] - s["ce"].mean()) <= float(s["b_ce"].max()) + 1e-12, name
        assert abs(printed[name]["val_loss2"] - s["se"].mean()) <= float(s["b_se"].max()) + 1e-12, name
        assert abs(printed[name]["pi_entropy"] - s["ent"].mean()) <= float(s["b_ent"].max()) + 1e-12, name
    r = subprocess.run([sys.executable, tool, "-t", traces[0], "--model1", "5:" + blob, "--model2", blob], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "residual blocks" in r.stderr
