"""CPU: the yardstick of the tower tests (tests/tower_ref.py) against the oracle network (oracle/nn.c), and the conditions that keep
the GPU tests (tests/test_gpu_tower.py) from passing vacuously.

The oracle runs the probe nets of forms (a) to (g) in its bf16- and fp8-emulating modes on 0-, 1- and 3-block nets (its latent is the
residual stream after the last block, so stage s of a net is the latent of the net cut after s blocks); its latents must lie inside
the bounds around the closed forms.  That pins the closed forms and the probes to an independent implementation before any GPU run.
The oracle sums in another order and normalises in float64, so the same bounds must hold for it: the probes are order-free.  On the
full position sets of the GPU tests, with no oracle in the loop: representability, exact sums, tie margins, bound ceilings, the share
of rows that form (d) leaves out and its coverage of (input channel, tap).  Last, three deliberately wrong blobs must FAIL."""
import numpy as np
import pytest

import scw
import tower_ref as tw
from helpers import golden_boards
from support import IDS, INST

MODE = {"bf16": dict(emulate_bf16=True), "fp8": dict(emulate_fp8=True)}
META = np.zeros(7, np.int32)


def _latents(orc, sd, n_blocks, C, prec, boards):
    """the oracle's latent [n][64][C] of the net made of sd's stem, its first n_blocks blocks and its heads"""
    net = orc.Net(n_blocks, C, seed=1, **MODE[prec])
    for i, (name, shape, _, _) in enumerate(scw.tensor_table(n_blocks, C)):
        net.set_tensor(i, sd[name])
    return np.stack([net.forward(b, META, latent=True)[2] for b in boards])


def _sub(chan, pix, k):
    """a spread of k positions of an impulse set, PIX6 and whole-board ones among them"""
    i = np.unique(np.linspace(0, len(chan) - 1, k).astype(int))
    return chan[i], pix[i]


# ---------------------------------------------------------------------------------- the oracle against the closed forms
@pytest.mark.parametrize("C,prec", INST, ids=IDS)
def test_oracle_stem_forms(orc, C, prec):
    """(a) and (b) on the 0-block net"""
    sd = tw.net_a(C, prec)
    tw.representable(sd, prec)
    pl, px = _sub(*tw.stem_positions(), 40)
    ref, bd = tw.form_a(sd, prec, pl, px)
    tw.compare(f"oracle {C} {prec} (a)", _latents(orc, sd, 0, C, prec, tw.impulse_board(pl, px)), ref, bd)
    sd = tw.net_b(C, prec)
    tw.representable(sd, prec)
    boards = tw.dense_boards(golden_boards())
    ref, bd = tw.form_b(sd, boards)
    tw.compare(f"oracle {C} {prec} (b)", _latents(orc, sd, 0, C, prec, boards), ref, bd)


@pytest.mark.parametrize("C,prec", INST, ids=IDS)
def test_oracle_conv_impulse_forms(orc, C, prec):
    """(c) and (d) on the 1-block net, through the last stem map (the one that is no identity)"""
    off = tw.sigmas(C)[-1]
    sd, v0, v1 = tw.net_c(C, prec, off)
    tw.representable(sd, prec)
    ch, px = _sub(*tw.conv_positions(C, 0), 24)
    ch = ch % 112 + off
    ref, bd = tw.form_c(sd, prec, 0, ch, px, v0[prec], v1[prec])
    tw.compare(f"oracle {C} {prec} (c)", _latents(orc, sd, 1, C, prec, tw.impulse_board(ch - off, px)), ref, bd)
    sd, v0 = tw.net_d(C, prec, off)
    tw.representable(sd, prec)
    ref, bd, keep, alts = tw.form_d(sd, prec, 0, ch, px, v0[prec])
    tw.compare(f"oracle {C} {prec} (d)", _latents(orc, sd, 1, C, prec, tw.impulse_board(ch - off, px)), ref, bd, keep, alts)


@pytest.mark.parametrize("C,prec", INST, ids=IDS)
def test_oracle_exact_sum_forms(orc, C, prec):
    """(e) for both convs and (f) on the 1-block net; the inputs differ, the latents must not"""
    boards = tw.dense_boards(golden_boards()[:1])
    sd, kap, kap1 = tw.net_e2(C, prec)
    tw.representable(sd, prec)
    lat = _latents(orc, sd, 1, C, prec, boards)
    ref, bd = tw.form_e2(sd, 0, kap, kap1)
    tw.compare(f"oracle {C} {prec} (e) conv2", lat, np.broadcast_to(ref, lat.shape), np.broadcast_to(bd, lat.shape))
    assert all(np.array_equal(lat[0], x) for x in lat)
    sd, kap = tw.net_e1(C, prec)
    tw.representable(sd, prec)
    lat = _latents(orc, sd, 1, C, prec, boards)
    ref, bd, keep, alts = tw.form_e1(sd, prec, 0, kap)
    tw.compare(f"oracle {C} {prec} (e) conv1", lat[:1], ref[None], bd[None], keep[None], alts)
    assert all(np.array_equal(lat[0], x) for x in lat)
    for bname in tw.betas(C):
        sd, kap, beta = tw.net_f(C, prec, bname)
        tw.representable(sd, prec)
        lat = _latents(orc, sd, 1, C, prec, boards[:2])
        ref, bd, _, _ = tw.form_f(sd, 0, kap, beta)
        tw.compare(f"oracle {C} {prec} (f) {bname}", lat, np.broadcast_to(ref, lat.shape), np.broadcast_to(bd, lat.shape))
        assert np.array_equal(lat[0], lat[1]) and all(np.array_equal(lat[0, 0], r) for r in lat[0])


@pytest.mark.parametrize("C,prec", INST, ids=IDS)
def test_oracle_block_position(orc, C, prec):
    """(g) on the 3-block net: form (c) in block k, the other two transparent: the latent is the closed form of stage k, and the net
    cut after k blocks gives the same bits"""
    ch, px = _sub(*tw.impulse_set([], range(112)), 6)
    for k in range(3):
        sd, v0, v1 = tw.net_c(C, prec, 0, nb=3, blk=k)
        tw.representable(sd, prec)
        boards = tw.impulse_board(ch, px)
        lat = _latents(orc, sd, 3, C, prec, boards)
        ref, bd = tw.form_c(sd, prec, k, ch, px, v0[prec], v1[prec])
        tw.compare(f"oracle {C} {prec} (g) block {k + 1}", lat, ref, bd)
        assert np.array_equal(lat, _latents(orc, sd, k + 1, C, prec, boards))


# ---------------------------------------------------------------------------------- conditions on the full position sets
def test_impulse_sets_reach_every_edge():
    for C in (128, 256):
        CT = C // 128
        c8 = np.asarray(tw.chan8(C))
        assert len(set(c8 // (32 * CT))) == 4 and len(set((c8 % (32 * CT)) // 32)) == CT          # waves, channel tiles
        assert len(set((c8 % 32) // 8)) == 4 and len(set((c8 % 8) // 4)) == 2                     # register quads, lane halves
        assert len(set(c8 // 16)) == 8
        seen = []
        for off in tw.sigmas(C):
            ch, px = tw.conv_positions(C, off)
            assert ((ch >= off) & (ch < off + 112)).all()
            seen += list(zip(ch, px))
        assert len(seen) == len(set(seen)) == 6 * (C - 8) + 8 * 64
        assert {c for c, p in seen} == set(range(C)) and {c // 16 for c, p in seen} == set(range(C // 16))
        assert all((c, p) in set(seen) for c in c8 for p in range(64))
    pl, px = tw.stem_positions()
    assert {0, 111} <= set(tw.PLANES8) and set(pl) == set(range(112)) and len(pl) == 8 * 64 + 104 * 6
    assert tw.PIX6 == (0, 7, 56, 63, 3 * 8 + 3, 4)


@pytest.mark.parametrize("C,prec", INST, ids=IDS)
def test_bounds_stay_under_the_ceiling(C, prec):
    """every bound of (a), (b), (c), (e), (f) on the GPU tests' own position sets is at most 1e-4 of its row's largest |reference|;
    the sums of (b), (e), (f) are exact in float32 in three orders"""
    worst = {}
    sd = tw.net_a(C, prec)
    pl, px = tw.stem_positions()
    worst["a"] = max(tw.row_ceiling(*tw.form_a(sd, prec, pl[s], px[s])) for s in tw.chunks(len(pl)))
    sd = tw.net_b(C, prec)
    boards = tw.dense_boards(golden_boards())
    worst["b"] = tw.row_ceiling(*tw.form_b(sd, boards))
    for b in boards[[0, -2, -1]]:
        assert tw.sums_are_exact(np.float64(b).reshape(1, 64, 112), sd["conv_block.0.weight"], sd["conv_block.0.bias"], (0, 7, 27, 60, 63))
    for off in tw.sigmas(C):
        sd, v0, v1 = tw.net_c(C, prec, off)
        ch, px = tw.conv_positions(C, off)
        worst["c"] = max([worst.get("c", 0)] + [tw.row_ceiling(*tw.form_c(sd, prec, 0, ch[s], px[s], v0[prec], v1[prec])) for s in tw.chunks(len(ch))])
    sd, kap, kap1 = tw.net_e2(C, prec)
    worst["e2"] = tw.row_ceiling(*tw.form_e2(sd, 0, kap, kap1))
    assert tw.sums_are_exact(np.broadcast_to(np.float64(kap1), (1, 64, C)), sd["res_blocks.0.conv2.weight"], sd["res_blocks.0.conv2.bias"], (0, 4, 7, 24, 27, 31, 56, 60, 63))
    sd, kap = tw.net_e1(C, prec)
    ref, bd, keep, alts = tw.form_e1(sd, prec, 0, kap)
    worst["e1"] = max(tw.row_ceiling(ref, bd, keep), tw.row_ceiling(alts[2], alts[3]) if len(alts[0]) else 0)
    keep = keep.copy()
    keep[alts[1]] = True                                         # held to a rounding variant
    assert tw.sums_are_exact(np.broadcast_to(np.float64(kap), (1, 64, C)), sd["res_blocks.0.conv1.weight"], sd["res_blocks.0.conv1.bias"], (0, 4, 7, 24, 27, 31, 56, 60, 63))
    # the 9 pixel classes (corner, edge, interior by rank and file): at least 6 compared, one of each kind among them
    cls = lambda p: (min(p // 8, 1) + (p // 8 == 7), min(p % 8, 1) + (p % 8 == 7))
    kept = {cls(p) for p in range(64) if keep[p]}
    assert len(kept) >= 6 and {(1, 1)} <= kept and kept & {(0, 0), (0, 2), (2, 0), (2, 2)} and kept & {(0, 1), (1, 0), (1, 2), (2, 1)}, kept
    for bname in tw.betas(C):
        sd, kap, beta = tw.net_f(C, prec, bname)
        ref, bd, hid, z = tw.form_f(sd, 0, kap, beta)            # asserts the exact sums and the bf16 hidden vector itself
        worst["f"] = max(worst.get("f", 0), tw.row_ceiling(ref[None], bd[None]))
        assert (hid > 0).any() and (hid == 0).sum() >= 8, bname  # hidden units on both sides of the ReLU
        assert (np.abs(z) < 0.5).any() and ((np.abs(z) > 1) & (np.abs(z) < 6)).any() and (z >= 40).any() and (z <= -40).any()
    print(f"{C} {prec}: largest bound / row maximum by form: " + ", ".join(f"({k}) {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= tw.CEIL, worst


@pytest.mark.parametrize("C,prec", INST, ids=IDS)
def test_form_d_leaves_few_rows_out_and_covers_every_tap(C, prec):
    """(d) on the full sets: at most 25 % of the (position, pixel) rows -- of all rows and of the rows next to the impulse -- are left
    out for rounding ties (a row with up to MAX_FLIPS elements on a tie is not left out: it is held to the nearest of its rounding
    variants), every (input channel, tap) pair that lies on the board keeps a compared row, the bounds of the compared rows,
    variants included, stay under the ceiling"""
    out_all, out_near, n_all, n_near, ceil, n_var = 0, 0, 0, 0, 0.0, 0
    for off in tw.sigmas(C):
        sd, v0 = tw.net_d(C, prec, off)
        ch, px = tw.conv_positions(C, off)
        pairs = {}
        for s in tw.chunks(len(ch)):
            ref, bd, keep, alts = tw.form_d(sd, prec, 0, ch[s], px[s], v0[prec])
            ceil = max(ceil, tw.row_ceiling(ref, bd, keep), tw.row_ceiling(alts[2], alts[3]) if len(alts[0]) else 0)
            n_var += len(alts[0])
            keep = keep.copy()
            keep[alts[0], alts[1]] = True
            nb = tw.neighbours(px[s])
            i, t = np.nonzero(nb >= 0)
            k = keep[i, nb[i, t]]
            out_all, n_all = out_all + (~keep).sum(), n_all + keep.size
            out_near, n_near = out_near + (~k).sum(), n_near + k.size
            for c, tap, kk in zip(ch[s][i], t, k):
                pairs[(c, tap)] = pairs.get((c, tap), False) or bool(kk)
        assert len(pairs) == 9 * len(set(ch)) and all(pairs.values()), [p for p, v in pairs.items() if not v][:10]
    print(f"{C} {prec} (d): rows left out {out_all / n_all:.2%} of all, {out_near / n_near:.2%} of those next to the impulse "
          f"({n_var / n_near:.2%} of these held to a rounding variant); largest bound / row maximum {ceil:.2e}")
    assert out_all <= 0.25 * n_all and out_near <= 0.25 * n_near and ceil <= tw.CEIL


# ---------------------------------------------------------------------------------- the probes see what they claim to see
def test_wrong_blobs_are_caught(orc):
    """a conv1 with two taps swapped, a conv2 with two input channels swapped, a stem with one k-16 group zeroed: the oracle, fed
    the wrong blob, must miss the closed form of the right one"""
    C, prec = 128, "bf16"

    def share(label, lat, ref, bd, keep=None, alts=None):
        try:
            return tw.compare(label, lat, ref, bd, keep, alts)
        except AssertionError:
            return np.inf

    ch, px = _sub(*tw.conv_positions(C, 0), 24)
    boards = tw.impulse_board(ch, px)
    sd, v0 = tw.net_d(C, prec, 0)
    ref, bd, keep, alts = tw.form_d(sd, prec, 0, ch, px, v0[prec])
    assert share("right conv1", _latents(orc, sd, 1, C, prec, boards), ref, bd, keep, alts) <= 1
    W = sd["res_blocks.0.conv1.weight"].copy()
    W[:, :, 0, 1], W[:, :, 2, 1] = W[:, :, 2, 1].copy(), W[:, :, 0, 1].copy()
    assert share("conv1, taps swapped", _latents(orc, dict(sd, **{"res_blocks.0.conv1.weight": W}), 1, C, prec, boards), ref, bd, keep, alts) > 1

    sd, v0, v1 = tw.net_c(C, prec, 0)
    ref, bd = tw.form_c(sd, prec, 0, ch, px, v0[prec], v1[prec])
    assert share("right conv2", _latents(orc, sd, 1, C, prec, boards), ref, bd) <= 1
    W = sd["res_blocks.0.conv2.weight"].copy()
    c1, c2 = sorted(set(ch))[:2]
    W[:, c1], W[:, c2] = W[:, c2].copy(), W[:, c1].copy()
    assert share("conv2, input channels swapped", _latents(orc, dict(sd, **{"res_blocks.0.conv2.weight": W}), 1, C, prec, boards), ref, bd) > 1

    for form in "ab":
        sd = tw.net_a(C, prec) if form == "a" else tw.net_b(C, prec)
        if form == "a":
            pl, px = np.asarray([3, 17, 30, 64]), np.asarray([27, 0, 63, 12])
            boards, (ref, bd) = tw.impulse_board(pl, px), tw.form_a(sd, prec, pl, px)
        else:
            boards = tw.dense_boards(golden_boards())
            ref, bd = tw.form_b(sd, boards)
        assert share(f"right stem ({form})", _latents(orc, sd, 0, C, prec, boards), ref, bd) <= 1
        W = sd["conv_block.0.weight"].copy()
        W[:, 16:32] = 0
        assert share(f"stem ({form}), k-16 group zeroed", _latents(orc, dict(sd, **{"conv_block.0.weight": W}), 0, C, prec, boards), ref, bd) > 1


# ---------------------------------------------------------------------------------- operand rounding at the decision points
import rounding_ref as rr  # noqa: E402


def test_r_act_is_nearest_even_after_the_clamp():
    """tower_ref.r_act against the brute-force rule (the nearest finite code of the table of all codes, ties to the even code, the
    clamp first) on every decision point of the rounding tests, both signs, the values beyond 448 and the zeros; the landmarks that
    DESIGN records; and every wrong rule of the tests differs from the right one somewhere on these points"""
    for fmt in tw.PRECS:
        v = np.concatenate([g for g, _ in rr.groups(fmt)])
        v = np.concatenate([v, -v, [0.0, -0.0]]).astype(np.float32)
        want, got = rr.convert(v, fmt), tw.r_act(v, fmt)
        print(f"{fmt}: r_act against the brute-force rule on {len(v)} points: {(want != got).sum()} mismatches")
        assert np.array_equal(want, got) and np.array_equal(np.signbit(want), np.signbit(got))
        assert len(v) == 2 + 2 * (3 * 126 + len(rr.BIG) if fmt == "fp8" else 3 * 3 * 128)
        for rule in rr.RULES[fmt]:
            bad = rr.convert(v, fmt, rule)
            assert ((bad != want) & ~(np.isnan(bad) & np.isnan(want))).any(), rule
    r8 = lambda x: float(tw.r_act(np.float32(x), "fp8"))
    assert r8(2.0 ** -10) == 0 and r8(3 * 2.0 ** -10) == 2.0 ** -8 and r8(7.5 * 2.0 ** -9) == 2.0 ** -6 and r8(2.0 ** -9) == 2.0 ** -9
    assert all(r8(x) == 448 and r8(-x) == -448 for x in rr.BIG) and len(rr.midpoints("fp8")) == 126
    assert np.isnan(rr.convert(np.float32(480), "fp8", "noclamp")) and rr.convert(np.float32(464), "fp8", "noclamp") == 448
    rb = lambda x: float(tw.r_act(np.float32(x), "bf16"))
    assert rb(1 + 2.0 ** -8) == 1 and rb(1 + 3 * 2.0 ** -8) == 1 + 2.0 ** -6 and rb(2 - 2.0 ** -8) == 2


@pytest.mark.parametrize("C,prec", INST, ids=IDS)
@pytest.mark.parametrize("site", ["1", "2", "3", "6p", "6h"])
def test_oracle_meets_the_rounding_forms_of_the_trunk(orc, site, C, prec):
    """rounding_ref.check_site on sites 1, 2, 3 and 6 (pool and hidden vector): all decision points of the site's operand format"""
    n = rr.check_site(orc, site, C, prec)
    assert n == (3 * 126 if rr.precisions(site, prec) == "fp8" else 3 * 3 * 128)


@pytest.mark.parametrize("prec", tw.PRECS)
@pytest.mark.parametrize("site", ["1", "2", "3", "6p", "6h"])
def test_wrong_rounding_rules_are_caught_in_the_trunk(orc, site, prec):
    """truncation, ties away from zero and, in e4m3, flushed subnormals, a clamp at 240 and no clamp: rounding_ref.check_wrong_rules"""
    rr.check_wrong_rules(orc, site, 128, prec)


# ---------------------------------------------------------------------------------- LayerNorm rows with a large common offset
import ln_offset_ref as lo  # noqa: E402
from support import GOLD  # noqa: E402

TRUNK_LN = ("stem", "ln1", "ln2")


@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("mode", list(lo.MODES))
def test_oracle_is_the_two_pass_layernorm_at_every_offset_in_the_trunk(orc, mode, C):
    """ln_offset_ref.check_oracle at the stem LayerNorm, LN1 and LN2: the oracle, two-pass in double, meets assertion 1 and
    assertion 2 on EVERY rung, in its fp32 mode and in both emulating modes"""
    lo.check_oracle(orc, C, mode, TRUNK_LN)


@pytest.mark.parametrize("C,prec", INST, ids=IDS)
def test_offset_probes_of_the_trunk_meet_their_conditions(C, prec):
    """rows exact in float32, no ReLU cut behind a lift, at most `cap` elements on a tie up to R_REQ, a wrong operand shows"""
    assert [r[0] for r in lo.rows()].count(64) == 8 and len(lo.rows()) == 25 and {r[1] for r in lo.rows()} == {1, -1}
    lo.check_conditions(C, prec, TRUNK_LN)


@pytest.mark.parametrize("C,prec", INST, ids=IDS)
def test_a_one_pass_layernorm_is_caught_in_the_trunk(C, prec):
    """ln_offset_ref.one_pass32 in place of the LayerNorm, every other layer exact: within the one-pass bound on every rung, the
    operation up to a break rung above R_REQ, not the operation from there on"""
    for site in TRUNK_LN:
        assert lo.check_wrong_ln(C, prec, site) in lo.RUNGS[2:]


def test_mean_over_sigma_of_the_projects_networks(orc):
    """R_REQ: the table of ln_offset_ref.RATIOS measured again with the oracle's float64 statistics, its
    largest entry, and the rung that follows from it"""
    got = lo.measure_ratios(orc, GOLD)
    assert set(got) == set(lo.RATIOS) == {n[0] for n in lo.NETWORKS}
    for name, want in lo.RATIOS.items():
        print(f"mean / sigma, {name}: " + ", ".join(f"{s} {got[name][s]:.3f}" for s in lo.LN_SITES))
        assert np.allclose([got[name][s] for s in lo.LN_SITES], want, rtol=0, atol=6e-4), name
    top = max(max(v) for v in lo.RATIOS.values())
    assert top == lo.LARGEST_RATIO and lo.required_rung(top) == lo.R_REQ
    assert all(env is None or env > lo.R_REQ for env in lo.ENVELOPE.values()) and len(lo.ENVELOPE) == 24
