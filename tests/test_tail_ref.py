"""CPU: the yardstick of the output-tail tests (tests/tail_ref.py) against the oracle network (oracle/nn.c, oracle/mcts.c).

The oracle runs the probe weights at both trunk widths and in its three modes; its log-probabilities, values and `orc_eval_net` priors
must lie inside the bound functions around the closed forms.  That pins the closed forms to an independent implementation (one that
runs the whole trunk in front of the tail, so a probe that did not remove the trunk would show) and shows that the bounds, which the
GPU tests use unchanged, are not already too tight for plain float32 libm arithmetic.  The probe editors are checked too: bfloat16
representability, the plane -> wave map of the softmax, exact ties within a plane."""
import ctypes as C
import os

import numpy as np
import pytest

import scw
import tail_ref as tr
from lines import WIDE
from support import GOLD

MODES = {0: {}, 1: dict(emulate_bf16=True), 2: dict(emulate_fp8=True)}
_CACHE = {}


def _inputs():
    """boards of a few golden rows and an all-zero board, cycled over the 130 rows of the meta grid"""
    g = np.load(os.path.join(GOLD, "nn_ref_b1_c256.npz"))
    boards = np.concatenate([g["boards"][[0, 3, 7]], np.zeros((1, 8, 8, 112), np.int8)])
    meta = tr.meta_grid()
    return boards[np.arange(len(meta)) % 4], meta


def _eval_roots(orc, net):
    """orc_eval_net on roots of 20, 82 and 218 legal moves -> [(width, action indices, priors, the net's logp row)]"""
    fn = orc.lib().orc_eval_net
    fn.restype, fn.argtypes = None, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    res = []
    for line, fen, width in (([], None, 20), (WIDE, None, 82), ([], tr.FEN218 % (98, 303), 218)):
        st = orc.State(fen)
        for m in line:
            st.push(m)
        moves = st.legal_moves()
        assert len(moves) == width and st.outcome() is None
        idx = np.asarray([orc.move_index(m, st.turn) for m in moves], np.int32)
        assert width != 218 or len(set(idx // 64)) == 23           # the 218 moves lie in 23 of the 73 move planes
        mv, pri, val = np.asarray(moves, np.uint16), np.zeros(width, np.float32), np.zeros(1, np.float32)
        fn(net.h, st.h, width, mv.ctypes.data, idx.ctypes.data, pri.ctypes.data, val.ctypes.data)
        logp, v = net.forward(*st.encode())
        assert v == val[0]
        res.append((width, idx, pri, logp))
    return res


def _run(orc, Cw, mode):
    """every bias pattern on 16-17 rows of the meta grid each, the two value probes alternating: name -> (logp rows, values, rows,
    value probe, orc_eval_net on three roots)"""
    if (Cw, mode) not in _CACHE:
        boards, meta = _inputs()
        table = [t[0] for t in scw.tensor_table(1, Cw)]
        net = orc.Net(1, Cw, seed=13, **MODES[mode])
        out = {}
        for k, (name, b) in enumerate(tr.bias_patterns().items()):
            vname = ("spread", "saturated")[k % 2]
            sd = tr.value_probe(tr.policy_probe(scw.prng_state_dict(1, Cw, 13), b), *tr.value_probes()[vname])
            for i, tname in enumerate(table):
                if tname.startswith("policy_head.model.3") or tname.startswith("value_head.ffn"):
                    net.set_tensor(i, sd[tname])
            rows = np.arange(k, len(meta), 8)
            res = [net.forward(boards[r], meta[r]) for r in rows]
            out[name] = (np.stack([x[0] for x in res]), np.asarray([x[1] for x in res], np.float32), rows, vname, _eval_roots(orc, net))
        _CACHE[(Cw, mode)] = (out, net)
    return _CACHE[(Cw, mode)]


def test_probe_editors_and_patterns():
    pats = tr.bias_patterns()
    assert list(pats) == ["flat", "levels", "wave0", "wave1", "wave2", "wave3", "far", "low"]
    lv = pats["levels"]
    assert len(set(lv)) == 73 and lv.min() == 0 and lv.max() == 32 and np.array_equal(lv * 4, np.rint(lv * 4))
    assert np.array_equal(pats["low"], lv - 64) and np.array_equal(tr.logp_closed(pats["low"]), tr.logp_closed(lv))
    assert pats["far"].max() == 96 and np.sort(pats["far"])[-2] <= 0
    for name, b in pats.items():
        sd = tr.policy_probe(scw.prng_state_dict(1, 128, 1), b)       # asserts bfloat16 representability
        assert not sd["policy_head.model.3.weight"].any() and np.array_equal(sd["policy_head.model.3.bias"], b.astype(np.float32))
        lp = tr.logp_closed(b)
        assert abs(np.exp(lp).sum() - 1) < 1e-12
        assert np.array_equal(lp.reshape(73, 64), np.repeat(lp[::64], 64).reshape(73, 64))      # exact ties within a plane
        # the maximum sits in the wave the pattern names: action a is read by thread a % 256, wave (a % 256) // 64 = plane % 4
        top = np.flatnonzero(lp == lp.max())
        assert np.array_equal((top % 256) // 64, tr.wave_of_plane(top // 64))
        if name.startswith("wave"):
            w = int(name[4])
            assert set((top % 256) // 64) == {w}
            mass = np.exp(lp).reshape(73, 64).sum(1)
            assert mass[np.arange(73) % 4 == w].sum() > 0.999             # the other three waves hold under 1e-3 of the mass
    with pytest.raises(AssertionError):
        tr.policy_probe({}, np.full(73, 0.1))                          # 0.1 is no bfloat16 value
    with pytest.raises(AssertionError):
        tr.policy_probe({}, np.full(73, 95.75))                        # nor is 95.75 (9 significant bits)
    grid = tr.meta_grid()
    assert grid.shape == (130, 7)
    for name, p in tr.value_probes().items():
        sd = tr.value_probe(scw.prng_state_dict(1, 128, 1), *p)
        assert not sd["value_head.ffn.0.weight"][:, :64 * 256].any() and sd["value_head.ffn.0.weight"][:, 64 * 256:].any()
        s = tr.value_args(grid, *p)
        if name == "spread":
            assert np.abs(s).max() < 3 and s.min() < -2 and s.max() > 2 and np.sum(np.abs(s) < 1) > 20
        else:
            assert s.min() >= 12
    # bfloat16 ties-to-even of meta: the cases the closed form depends on
    assert list(tr.bf16_rne(np.float32([257, 259, 301, 303, 511, 513, 1023]))) == [256, 260, 300, 304, 512, 512, 1024]


def test_bounds_stay_below_their_ceilings():
    """the conditions of the bound model: logp below 1e-4 absolute wherever |logp| <= 40, priors below 1e-4 relative"""
    rng = np.random.default_rng(2)
    for name, b in tr.bias_patterns().items():
        lp, bd = tr.logp_closed(b), tr.logp_bound(b)
        assert bd[np.abs(lp) <= 40].max() < tr.CEIL_LOGP, name
        for n in tr.WIDTHS:
            for sname, idx in tr.index_sets(lp, n, rng).items():
                assert len(set(idx)) == n
                _, rel = tr.prior_bound(lp, idx, bd[idx])
                assert rel.max() < tr.CEIL_PRIOR, (name, n, sname)
        print(f"{name}: logp bound {bd[np.abs(lp) <= 40].max():.2e} at |logp| <= 40 ({bd.max():.2e} overall, min logp {lp.min():.1f})")


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["fp32", "bf16", "fp8"])
@pytest.mark.parametrize("Cw", [128, 256])
def test_oracle_logp_equals_the_closed_form(orc, Cw, mode):
    out, _ = _run(orc, Cw, mode)
    worst = (0.0, 0.0)
    for name, b in tr.bias_patterns().items():
        lp = out[name][0]
        ref, bd = tr.logp_closed(b), tr.logp_bound(b)
        assert all(np.array_equal(r.view(np.uint32), lp[0].view(np.uint32)) for r in lp), name          # the probe removes the input
        assert np.array_equal(lp[0].reshape(73, 64), np.repeat(lp[0][::64], 64).reshape(73, 64)), name  # ties within a plane
        err = np.abs(lp[0].astype(np.float64) - ref)
        worst = max(worst, (float((err / bd).max()), float(err.max())))
        assert (err <= bd).all(), (name, err.max(), bd[np.argmax(err / bd)])
    print(f"C={Cw} mode {mode}: max |logp - closed form| {worst[1]:.2e}, at most {worst[0]:.3f} of its bound")


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["fp32", "bf16", "fp8"])
@pytest.mark.parametrize("Cw", [128, 256])
def test_oracle_value_equals_the_closed_form(orc, Cw, mode):
    """the fp32 mode feeds meta unrounded, the emulating modes round it to bfloat16 (ties to even) as the engine does"""
    out, _ = _run(orc, Cw, mode)
    meta = tr.meta_grid()
    worst = {}
    for name, (_, val, rows, vname, _) in out.items():
        p = tr.value_probes()[vname]
        ref = tr.value_closed(meta[rows], *p, round_meta=mode > 0)
        bd = tr.value_bound(meta[rows], *p, k_fc2=tr.K_FC2_ORACLE, round_meta=mode > 0)
        err = np.abs(val.astype(np.float64) - ref)
        assert (err <= bd).all(), (name, vname, err.max(), bd[np.argmax(err / bd)])
        worst[vname] = max(worst.get(vname, (0, 0)), (float(err.max()), float(bd[np.argmax(err)])))
        if mode > 0 and vname == "spread":   # the rounding of meta is visible: the unrounded closed form is far outside the bound
            far = np.abs(tr.value_closed(meta[rows], *p, round_meta=False) - ref)
            moved = (tr.bf16_rne(meta[rows].astype(np.float32)) != meta[rows]).any(1)
            assert moved.sum() >= 4 and (far[moved] > 2 * bd[moved]).all()
    for vname, (e, bnd) in worst.items():
        print(f"C={Cw} mode {mode} {vname}: max |value - closed form| {e:.2e} (bound {bnd:.2e})")


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["fp32", "bf16", "fp8"])
@pytest.mark.parametrize("Cw", [128, 256])
def test_oracle_priors_equal_the_definition_on_its_own_logp(orc, Cw, mode):
    """orc_eval_net (the evaluator of the oracle's search) on roots of 20, 82 and 218 moves against priors_from_logp of the oracle's
    own log-probabilities: float32 libm expf and a sequential float32 sum (up to 218 roundings) in place of the device's tree"""
    out, _ = _run(orc, Cw, mode)
    for name in tr.bias_patterns():
        for width, idx, pri, logp in out[name][4]:
            ref = tr.priors_from_logp(logp, idx)
            bd, _ = tr.prior_bound(logp, idx)
            bd = bd + (width - tr.K_PRIOR_SUM) * tr.U * ref      # the sequential sum's roundings beyond the device tree's 9
            err = np.abs(pri.astype(np.float64) - ref)
            assert (err <= bd).all() and pri.sum(dtype=np.float64) <= 1, (name, width)
            if name == "levels":
                print(f"C={Cw} mode {mode} {name} width {width}: max rel prior error {(err / ref).max():.2e} (bound {(bd / ref).max():.2e})")
