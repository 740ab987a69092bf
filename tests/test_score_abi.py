"""Scoring networks on device tensors, checks that need no GPU: sc_forward_device / sc_score_positions / sc_compare_engines are
declared, bound and exported; bad arguments are refused before anything touches a device; without a device each call fails
loudly; the numpy yardstick of the GPU tests (tests/score_ref.py) equals the reference's formulas in torch on the CPU; and
tools/validate_model.py takes the reference script's command line."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import score_ref
from support import ROOT, _p, scamd_built  # noqa: F401

NEW = {"sc_forward_device": 7, "sc_score_positions": 15, "sc_compare_engines": 9}


def test_new_symbols_are_declared_bound_and_exported(scamd):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sc_engine.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", scamd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TW"}
    for name, n_args in NEW.items():
        m = re.search(rf"\b{name}\s*\((.*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_args, name
        assert len(scamd.binding.ABI[name][1]) == n_args, name
        assert name in exported, name
    for name in ("score_torch", "compare_torch"):
        assert callable(getattr(scamd, name))
    assert callable(scamd.Engine.forward_torch)
    # the summaries are plain double arrays: the header declares no struct for them
    assert len(re.findall(r"typedef\s+struct\s*\{", hdr)) == 4


def test_bad_arguments_are_refused_before_the_device(scamd):
    """-1 with a message, with or without a GPU: these checks come first.  The engine handle is never dereferenced by them, so a
    stand-in address serves where no GPU can build one"""
    L = scamd.lib()
    eng = C.c_void_p(0x1000)
    b, m = np.zeros((1, 8, 8, 112), np.int8), np.zeros((1, 7), np.int32)
    d, dl, li, nl = np.zeros((1, 4672), np.float32), np.zeros((1, 224), np.float32), np.zeros((1, 224), np.uint16), np.zeros(1, np.int32)
    oc, out = np.zeros(1, np.float32), np.zeros(1, np.float32)
    summ = np.zeros(9, np.float64)
    err = lambda: L.sc_last_error().decode()
    # both dist forms / neither / half of the sparse form
    assert L.sc_score_positions(eng, 1, _p(b), _p(m), _p(d), _p(dl), _p(li), _p(nl), _p(oc), None, _p(out), None, None, None, _p(summ)) == -1
    assert "ONE form" in err()
    assert L.sc_score_positions(eng, 1, _p(b), _p(m), None, None, None, None, _p(oc), None, _p(out), None, None, None, _p(summ)) == -1
    assert "missing" in err()
    assert L.sc_score_positions(eng, 1, _p(b), _p(m), None, _p(dl), None, _p(nl), _p(oc), None, _p(out), None, None, None, _p(summ)) == -1
    # NULL boards, n < 0, NULL engine, NULL outcome
    assert L.sc_score_positions(eng, 1, None, _p(m), _p(d), None, None, None, _p(oc), None, _p(out), None, None, None, _p(summ)) == -1
    assert L.sc_score_positions(eng, -1, _p(b), _p(m), _p(d), None, None, None, _p(oc), None, _p(out), None, None, None, _p(summ)) == -1
    assert L.sc_score_positions(None, 1, _p(b), _p(m), _p(d), None, None, None, _p(oc), None, _p(out), None, None, None, _p(summ)) == -1
    assert L.sc_score_positions(eng, 1, _p(b), _p(m), _p(d), None, None, None, None, None, _p(out), None, None, None, _p(summ)) == -1
    assert L.sc_forward_device(eng, 1, None, _p(m), None, None, _p(out)) == -1
    assert L.sc_forward_device(eng, -1, _p(b), _p(m), None, None, _p(out)) == -1
    assert L.sc_forward_device(eng, 1, _p(b), _p(m), None, None, None) == -1
    assert L.sc_forward_device(None, 1, _p(b), _p(m), None, None, _p(out)) == -1
    assert L.sc_compare_engines(eng, eng, 1, None, _p(m), None, _p(out), None, _p(summ)) == -1
    assert L.sc_compare_engines(eng, eng, -1, _p(b), _p(m), None, _p(out), None, _p(summ)) == -1
    assert L.sc_compare_engines(eng, None, 1, _p(b), _p(m), None, _p(out), None, _p(summ)) == -1
    assert "bad argument" in err()


def test_fails_loudly_without_gpu(scamd):
    L = scamd.lib()
    if L.sc_device_count() > 0:
        pytest.skip("a GPU is present")
    eng = C.c_void_p(0x1000)   # never dereferenced: the device count is asked first
    b, m = np.zeros((1, 8, 8, 112), np.int8), np.zeros((1, 7), np.int32)
    d, oc, out = np.zeros((1, 4672), np.float32), np.zeros(1, np.float32), np.zeros(1, np.float32)
    summ = np.zeros(9, np.float64)
    assert L.sc_forward_device(eng, 1, _p(b), _p(m), None, None, _p(out)) == -3 and "no HIP device" in L.sc_last_error().decode()
    rc = L.sc_score_positions(eng, 1, _p(b), _p(m), _p(d), None, None, None, _p(oc), None, _p(out), None, None, None, _p(summ))
    assert rc == -3 and "no HIP device" in L.sc_last_error().decode()
    rc = L.sc_compare_engines(eng, eng, 1, _p(b), _p(m), None, _p(out), None, _p(summ))
    assert rc == -3 and "no HIP device" in L.sc_last_error().decode()
    with pytest.raises(scamd.EngineError, match="no HIP device"):
        scamd.score_torch(None, {})
    with pytest.raises(scamd.EngineError, match="no HIP device"):
        scamd.compare_torch(None, None, {})


def _rows(rng, P, sharp):
    z = rng.standard_normal((P, 4672)) * sharp
    z -= z.max(1, keepdims=True)
    return (z - np.log(np.exp(z).sum(1, keepdims=True))).astype(np.float32)


def _sparse(rng, P):
    """visit shares as the encoder leaves them: n_legal distinct actions per row, some with share 0, action 0 legal in every
    third row (once with a share, once with share 0), padding = action 0 with share 0"""
    li = np.zeros((P, 224), np.uint16)
    dl = np.zeros((P, 224), np.float32)
    nl = rng.integers(1, 219, P).astype(np.int32)
    nl[0] = 218
    for p in range(P):
        n = int(nl[p])
        acts = rng.choice(np.arange(1, 4672), n, replace=False)
        if p % 3 == 0:
            acts[rng.integers(0, n)] = 0
        cnt = rng.integers(0, 50, n).astype(np.float32)
        cnt[rng.integers(0, n)] += 1
        if p % 6 == 0:
            cnt[acts == 0] = 0
        li[p, :n] = acts
        dl[p, :n] = cnt / np.float32(cnt.sum() + 1e-5)
    return dl, li, nl


def test_yardstick_equals_the_reference_formulas_in_torch():
    import torch   # (a missing torch is a failure here, not a reason to skip)
    F = torch.nn.functional
    rng = np.random.default_rng(3)
    P = 24
    for sharp in (1.0, 6.0):
        logp, logp2 = _rows(rng, P, sharp), _rows(rng, P, sharp)
        dl, li, nl = _sparse(rng, P)
        dist = score_ref.dense_from_sparse(dl, li, nl)
        assert (dist[::3, 0] > 0).any() and (dist[::6, 0] == 0).all() and ((dl == 0) & (np.arange(224)[None] < nl[:, None])).any()
        # ... and equals torch's scatter_add_ over the whole rows (the padding adds 0 to action 0)
        t_dense = torch.zeros(P, 4672).scatter_add_(1, torch.from_numpy(li.astype(np.int64)), torch.from_numpy(dl))
        assert np.array_equal(t_dense.numpy().view(np.uint32), dist.view(np.uint32))
        value = np.tanh(rng.standard_normal(P)).astype(np.float32)
        value2 = np.tanh(rng.standard_normal(P)).astype(np.float32)
        outcome = rng.integers(-1, 2, P).astype(np.float32)
        r = score_ref.score(logp, value, dist, outcome)
        tl, td = torch.from_numpy(logp).double(), torch.from_numpy(dist).double()
        tv_, to = torch.from_numpy(value).double(), torch.from_numpy(outcome).double()
        loss1 = -(tl * td).sum() / P                                   # train.py compute_loss1
        loss2 = F.mse_loss(tv_, to)                                    # train.py compute_loss2
        pi_entropy = -(torch.exp(tl) * tl).sum(1).mean()               # train.py training_step
        assert abs(r["ce"].mean() - float(loss1)) <= 1e-13 * abs(float(loss1))
        assert abs(r["se"].mean() - float(loss2)) <= 1e-13 * abs(float(loss2))
        assert abs(r["ent"].mean() - float(pi_entropy)) <= 1e-13 * abs(float(pi_entropy))
        assert np.allclose(r["ce"], -(tl * td).sum(1).numpy(), rtol=1e-13, atol=0)
        c = score_ref.compare(logp, value, logp2, value2)
        p1, p2 = torch.exp(tl), torch.exp(torch.from_numpy(logp2).double())
        for p in range(P):
            assert abs(c["tv"][p] - float(torch.abs(p1[p] - p2[p]).sum() / 2)) <= 1e-14     # validate_model.py
        assert np.array_equal(c["dv"], torch.abs(tv_ - torch.from_numpy(value2).double()).numpy())
        # the bounds are what the docstring says, and small against the quantities
        assert (r["b_ce"] < 1e-4 * np.abs(r["ce"]) + 1e-12).all() and (r["b_ent"] < 1e-3).all() and (c["b_tv"] < 1e-5).all()
    # a zero share in front of a -inf log-probability stays out of the sum (torch's 0 * -inf would be NaN)
    lp = np.full((1, 4672), -np.inf, np.float32)
    lp[0, 5] = 0.0
    d = np.zeros((1, 4672), np.float32)
    d[0, 5] = 1.0
    with np.errstate(invalid="ignore"):   # (the row's entropy is 0 * -inf: not what is looked at here)
        assert score_ref.score(lp, np.zeros(1, np.float32), d, np.zeros(1, np.float32))["ce"][0] == 0.0


def test_validate_model_tool_takes_the_reference_flags():
    tool = os.path.join(ROOT, "tools", "validate_model.py")
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--model1" in r.stdout and "--trace" in r.stdout, r.stderr[-2000:]
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import validate_model
    a = validate_model.parser().parse_args(["-t", "a.json", "b.json", "--model1", "5:one.scw", "--model2", "two.scw"])
    assert a.trace == ["a.json", "b.json"] and a.model1 == "5:one.scw" and a.model2 == "two.scw"
    assert validate_model.model_spec("5:one.scw") == (5, "one.scw") and validate_model.model_spec("two.scw") == (None, "two.scw")
    a = validate_model.parser().parse_args(["--trace", "a.json", "--model1", "x", "--model2", "y", "--precision2", "fp8", "--losses"])
    assert a.precision1 == "bf16" and a.precision2 == "fp8" and a.losses
