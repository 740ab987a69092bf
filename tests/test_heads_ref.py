"""CPU: the yardstick of the head tests (tests/heads_ref.py) against the oracle network (oracle/nn.c), and the conditions that keep the
GPU tests (tests/test_gpu_heads.py) from passing vacuously.

The oracle runs the probe nets in its three modes: its values and log-probabilities must lie inside the bounds around the closed
forms, under the ceiling of 1e-4 of the row's largest reference in every mode (the fp32 mode rounds no operand: its pattern
LayerNorms are exact by the bias g 2^-21; the emulating modes guard the probes against the fp8 clamp and the power-of-two channel
scales).  On the
full position sets of the GPU tests, with no oracle in the loop: balance of every +- row, exactness of every sum and the tie
margins (asserted inside the forms), the separation of the 16384 feature columns, the bound ceilings, and that one grid unit in a
single FC1 output moves the value by a hundred bounds.  Last, six deliberately wrong nets must FAIL the comparison."""
import numpy as np
import pytest

import heads_ref as hr
import rounding_ref as rr
import scw
import tail_ref as tr
import tower_ref as tw
from helpers import golden_boards
from support import IDS, INST

MODE = {"fp32": {}, "bf16": dict(emulate_bf16=True), "fp8": dict(emulate_fp8=True)}


def _oracle(orc, sd, nb, C, mode, boards, meta):
    """-> (logp[n,4672], value[n]) of the oracle net made of sd"""
    net = orc.Net(nb, C, seed=1, **MODE[mode])
    for i, (name, _, _, _) in enumerate(scw.tensor_table(nb, C)):
        net.set_tensor(i, sd[name])
    res = [net.forward(b, m) for b, m in zip(boards, meta)]
    return np.stack([r[0] for r in res]), np.asarray([r[1] for r in res], np.float32)


def _subset(n_imp, n_rand):
    """a spread of lone impulses (first and last plane and pixel among them), the dense set and a few multi-impulse boards"""
    imp = hr.impulse_positions()
    i = np.unique(np.linspace(0, len(imp) - 1, n_imp).astype(int))
    b = np.concatenate([imp[i], tw.dense_boards(golden_boards()), hr.random_boards(n_rand)])
    return b, hr.metas(len(b))


def _full_value_set():
    b = np.concatenate([hr.impulse_positions(), tw.dense_boards(golden_boards()), hr.random_boards(6)])
    return b, hr.metas(len(b))


def _policy_set():
    imp = hr.impulse_positions()
    return np.concatenate([hr.random_boards(16), tw.dense_boards(golden_boards()), imp[[0, 1000, 3333, 7167]]])


# ---------------------------------------------------------------------------------- the oracle against the closed forms
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp8"])
@pytest.mark.parametrize("C", [128, 256])
def test_oracle_heads_equal_the_closed_forms(orc, C, mode):
    """forms (v) and (p) on the 0-block net, every probe net and the one with a large plane 72; the net with one transparent block
    gives the same bits (r)"""
    prec = "bf16" if mode == "fp32" else mode
    boards, meta = _subset(20, 3)
    assert set(meta[:, 0]) == {0, 1}
    for k, big72 in ((0, False), (1, False), (2, False), (0, True)):
        sd = hr.net(C, prec, k, nb=0, big72=big72)
        lp, v = _oracle(orc, sd, 0, C, mode, boards, meta)
        ref, bd, _ = hr.form_v(sd, C, mode, boards, meta, k_fc2=tr.K_FC2_ORACLE)
        tw.compare(f"oracle {C} {mode} (v) net {k}{' big72' if big72 else ''}", v, ref, bd)
        assert bd.max() <= tw.CEIL * np.abs(ref).max()
        ref, bd = hr.form_p(sd, C, mode, boards)
        tw.compare(f"oracle {C} {mode} (p) net {k}{' big72' if big72 else ''}", lp, ref, bd)
        assert (bd.max(1) <= tw.CEIL * np.abs(ref).max(1)).all()
        if k == 1:
            sd1 = hr.net(C, prec, k, nb=1)
            lp1, v1 = _oracle(orc, sd1, 1, C, mode, boards[:4], meta[:4])
            assert np.array_equal(lp1, lp[:4]) and np.array_equal(v1, v[:4])


# ---------------------------------------------------------------------------------- conditions on the full position sets
@pytest.mark.parametrize("C,prec", INST, ids=IDS)
def test_probe_properties_on_the_full_sets(C, prec):
    """on the GPU tests' own sets: every +- row balanced, every sum exact, every rounded element TIE_SAFETY bounds from a tie (the
    forms assert these on every row), no bound above 1e-4 of its row's largest reference, |FC2 sum| < 1, one grid unit in a single
    h[j] worth MIN_RATIO bounds, every multi-impulse board with a reference row of its own at every pixel, in every net"""
    boards, meta = _full_value_set()
    pol = _policy_set()
    for k in range(len(hr.nets(C))):
        ceil_p = 0.0
        for big72 in ((False, True) if k == 0 else (False,)):
            lp, bd = hr.form_p(hr.net(C, prec, k, big72=big72), C, prec, pol)
            ceil_p = max(ceil_p, (bd.max(1) / np.abs(lp).max(1)).max())
            rows = [hr.distinct_pixel_rows(r) for r in lp[:16]]
            assert ceil_p <= tw.CEIL and min(rows) == 64, (k, ceil_p, rows)
        sd = hr.net(C, prec, k)
        v, bd, h = hr.form_v(sd, C, prec, boards, meta)
        ratio, smax = hr.unit_ratio(sd, v, bd)
        print(f"{C} {prec} net {k}: value bound / largest |value| {bd.max() / np.abs(v).max():.2e}, logp bound / row maximum {ceil_p:.2e}, "
              f"|FC2 sum| <= {smax:.2f}, a grid unit in one h[j] moves the value by >= {ratio:.0f} bounds, |h| <= {np.abs(h).max():.1f}")
        assert bd.max() <= tw.CEIL * np.abs(v).max() and smax < 1 and ratio >= hr.MIN_RATIO
        assert set(meta[:, 0]) == {0, 1} and (v != 0).all()           # both signs of the last factor, on values that show it


@pytest.mark.parametrize("C", [128, 256])
def test_feature_columns_are_separated(C):
    """over the union of the nets every one of the 16384 feature columns is active in some position and inactive in another, and no
    two columns share their activity vector in every net: a swapped column pair changes h somewhere.  The FC1 columns themselves are
    all distinct, and so are the 128 weights of FC2"""
    boards, _ = _full_value_set()
    keys, on, off = [], np.zeros(64 * hr.HEAD, bool), np.zeros(64 * hr.HEAD, bool)
    for k in range(len(hr.nets(C))):
        sd = hr.net(C, "bf16", k)
        act = hr.activity(sd, C, boards)
        on |= act.any(0)
        off |= (~act).any(0)
        keys.append(np.packbits(act.T, axis=-1))
        W1 = sd["value_head.ffn.0.weight"][:, :64 * hr.HEAD]
        assert len(np.unique(np.packbits(W1.T > 0, axis=-1), axis=0)) == 64 * hr.HEAD and (W1 != 0).all()
        assert len(set(sd["value_head.ffn.2.weight"].ravel())) == 128
    keys = np.ascontiguousarray(np.concatenate(keys, axis=1))
    distinct = len(np.unique(keys.view(np.dtype((np.void, keys.shape[1]))).ravel()))
    assert on.all() and off.all() and distinct == 64 * hr.HEAD, (on.sum(), off.sum(), distinct)


# ---------------------------------------------------------------------------------- the probes see what they claim to see
@pytest.mark.parametrize("C,mode", [(128, "bf16"), (256, "fp8"), (128, "fp32")], ids=["128_bf16", "256_fp8", "128_fp32"])
def test_wrong_nets_are_caught(orc, C, mode):
    """two FC1 columns exchanged, one 256-column K chunk of FC1 zeroed, two conv2 input channels exchanged, one value-conv pair moved
    to the neighbouring output pair, one value-conv weight read from the neighbouring slot, two pixels exchanged in the logits: the
    oracle, fed the wrong net, must miss the closed form of the right one"""
    boards, meta = _subset(20, 3)
    sd = hr.net(C, "bf16" if mode == "fp32" else mode, 1, nb=0)
    ref_v, bd_v, _ = hr.form_v(sd, C, mode, boards, meta, k_fc2=tr.K_FC2_ORACLE)
    ref_p, bd_p = hr.form_p(sd, C, mode, boards)

    def share(label, got, ref, bd):
        try:
            return tw.compare(label, got, ref, bd)
        except AssertionError:
            return np.inf

    def run(label, **wrong):
        lp, v = _oracle(orc, dict(sd, **wrong), 0, C, mode, boards, meta)
        return share(label + " (v)", v, ref_v, bd_v), share(label + " (p)", lp, ref_p, bd_p), lp

    sv, sp, lp = run("right net")
    assert sv <= 1 and sp <= 1
    act = hr.activity(sd, C, boards)
    W1 = sd["value_head.ffn.0.weight"].copy()
    a = 5 * 64 + 9                                               # a column and one whose activity differs on the set
    b = next(c for c in range(a + 1, 64 * hr.HEAD) if (act[:, c] != act[:, a]).any())
    W1[:, [a, b]] = W1[:, [b, a]]
    assert run("FC1, two columns exchanged", **{"value_head.ffn.0.weight": W1})[0] > 1
    W1 = sd["value_head.ffn.0.weight"].copy()
    W1[:, 37 * 256:38 * 256] = 0
    assert run("FC1, one K chunk zeroed", **{"value_head.ffn.0.weight": W1})[0] > 1
    W2 = sd["policy_head.model.2.weight"].copy()
    W2[:, [6, 9]] = W2[:, [9, 6]]
    assert run("conv2, two input channels exchanged", **{"policy_head.model.2.weight": W2})[1] > 1
    Wv, bv = sd["value_head.conv.0.weight"].copy(), sd["value_head.conv.0.bias"].copy()
    Wv[[10, 11, 12, 13]], bv[[10, 11, 12, 13]] = Wv[[12, 13, 10, 11]], bv[[12, 13, 10, 11]]
    assert run("value conv, one pair moved", **{"value_head.conv.0.weight": Wv, "value_head.conv.0.bias": bv})[0] > 1
    Wv = sd["value_head.conv.0.weight"].copy()
    c = next(c for c in range(40, C - 1) if Wv[17, c] != Wv[17, c + 1])
    Wv[17, c] = Wv[17, c + 1]
    assert run("value conv, one weight read from the neighbouring slot", **{"value_head.conv.0.weight": Wv})[0] > 1
    moved = lp.reshape(len(lp), 73, 64).copy()
    moved[:, :, [20, 21]] = moved[:, :, [21, 20]]
    assert share("logits, two pixels exchanged", moved.reshape(len(lp), -1), ref_p, bd_p) > 1


# ---------------------------------------------------------------------------------- operand rounding at the decision points
@pytest.mark.parametrize("C,prec", INST, ids=IDS)
@pytest.mark.parametrize("site", ["4", "5"])
def test_oracle_meets_the_rounding_forms_of_the_heads(orc, site, C, prec):
    """rounding_ref.check_site on site 4 (policy LayerNorm -> policy conv2, the one signed conversion: both signs of every e4m3
    decision point) and site 5 (value LayerNorm -> bf16 features, bf16 at both precisions)"""
    n = rr.check_site(orc, site, C, prec)
    assert n == (2 * 3 * 126 if rr.precisions(site, prec) == "fp8" else 3 * 3 * 128)


@pytest.mark.parametrize("prec", tw.PRECS)
@pytest.mark.parametrize("site", ["4", "5"])
def test_wrong_rounding_rules_are_caught_in_the_heads(orc, site, prec):
    """truncation, ties away from zero and, in e4m3, flushed subnormals, a clamp at 240 and no clamp: rounding_ref.check_wrong_rules"""
    rr.check_wrong_rules(orc, site, 128, prec)


# ---------------------------------------------------------------------------------- LayerNorm rows with a large common offset
import ln_offset_ref as lo  # noqa: E402

HEAD_LN = ("p73", "vln", "pln1")


@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("mode", list(lo.MODES))
def test_oracle_is_the_two_pass_layernorm_at_every_offset_in_the_heads(orc, mode, C):
    """ln_offset_ref.check_oracle at the 73-wide policy LayerNorm (padded channels add nothing, 1 / 73 is rounded), the value
    head's LayerNorm and the policy head's first: assertion 1 and assertion 2 on EVERY rung, in the oracle's three modes"""
    lo.check_oracle(orc, C, mode, HEAD_LN)


@pytest.mark.parametrize("C,prec", INST, ids=IDS)
def test_offset_probes_of_the_heads_meet_their_conditions(C, prec):
    """rows exact in float32, no ReLU cut behind a lift, at most `cap` elements on a tie up to R_REQ, a wrong operand shows"""
    lo.check_conditions(C, prec, HEAD_LN)


@pytest.mark.parametrize("C,prec", INST, ids=IDS)
def test_a_one_pass_layernorm_is_caught_in_the_heads(C, prec):
    """ln_offset_ref.one_pass32 in place of the LayerNorm, every other layer exact: within the one-pass bound on every rung, the
    operation up to a break rung above R_REQ, not the operation from there on"""
    for site in HEAD_LN:
        assert lo.check_wrong_ln(C, prec, site) in lo.RUNGS[2:]
