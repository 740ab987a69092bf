"""GPU (-m gpu): the trunk of the network -- stem conv, the two 3x3 convs of every residual block, their LayerNorms, squeeze-excitation
-- against float64 closed forms on probe weights (tests/tower_ref.py), at the four instantiations of the tower.

`Engine.debug` returns the fp32 residual stream of the stand-alone tower after the stem (stage 0), after block b (stage b) and at
the end (stage 1000).  Impulse probes put one non-zero operand into the conv under test, so every output is one product plus the
bias: a weight read from the wrong tap, channel or pixel shows at full size.  Exact-sum probes draw operands from dyadic grids, so
the K loop's sum is exact in any order: a k-step skipped, doubled or fed a stale fragment moves the result by whole grid units.  The
bounds are a handful of float32 roundings counted from the code; tests/test_tower_ref.py holds the CPU oracle to the same closed
forms and bounds and checks that no bound exceeds 1e-4 of its row's maximum.  Engines are built from weight blobs, one per probe net.

Every comparison prints its measured maximum, the bound at that element and the largest share of a bound that was used."""
from contextlib import closing

import numpy as np
import pytest

import tower_ref as tw
from helpers import golden_boards
from support import IDS, INST, engine_from_state, scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu


def _debug(eng, boards, stage):
    n = len(boards)
    assert n <= eng.L.sc_engine_max_batch(eng.h)
    out = eng.debug(boards, np.zeros((n, 7), np.int32), stage)
    assert np.isfinite(out).all()
    return out


def bits_zero_folded(a):
    """the bits of a float32 array with -0 read as +0 (ReLU is one v_max_f32, which may keep the sign of a zero)"""
    return (np.ascontiguousarray(a, np.float32) + np.float32(0)).view(np.uint32)


def _dense(n):
    """n differing inputs for the probes that remove the input"""
    b = tw.dense_boards(golden_boards())
    return b[np.arange(n) % len(b)]


def _chunked(label, got, form, n):
    """compare got[n,64,C] with form(slice) -> (ref, bound[, keep, alts]) chunk by chunk"""
    top = 0.0
    for s in tw.chunks(n):
        top = max(top, tw.compare(f"{label} [{s.start}:{s.stop}]", got[s], *form(s)))
    print(f"{label}: largest share of a bound over {n} positions {top:.3f}")


# ---------------------------------------------------------------------------------- a, b: the stem
@pytest.mark.parametrize("C,prec", INST, ids=IDS)
def test_stem_impulse(scamd, tmp_path, C, prec):
    """(a) a single 1 at (plane, pixel) under natural stem weights: every pixel for 8 planes, six pixels for all 112"""
    sd = tw.net_a(C, prec)
    pl, px = tw.stem_positions()
    with closing(engine_from_state(scamd, tmp_path, sd, 1, C, prec)) as eng:
        got = _debug(eng, tw.impulse_board(pl, px), 0)
    _chunked(f"{C} {prec} (a)", got, lambda s: tw.form_a(sd, prec, pl[s], px[s]), len(pl))


@pytest.mark.parametrize("C,prec", INST, ids=IDS)
def test_stem_exact_sums(scamd, tmp_path, C, prec):
    """(b) grid stem weights on golden positions, an all-ones and an all-zero board"""
    sd = tw.net_b(C, prec)
    boards = tw.dense_boards(golden_boards())
    with closing(engine_from_state(scamd, tmp_path, sd, 1, C, prec)) as eng:
        got = _debug(eng, boards, 0)
    tw.compare(f"{C} {prec} (b)", got, *tw.form_b(sd, boards))
    assert all(np.array_equal(bits_zero_folded(got[-1, 0]), bits_zero_folded(r)) for r in got[-1])       # the all-zero board: every pixel the bias row


# ---------------------------------------------------------------------------------- c, d: the block convs, impulses
@pytest.mark.parametrize("C,prec", INST, ids=IDS)
def test_conv2_impulse(scamd, tmp_path, C, prec):
    """(c) pass-through stem and conv1, natural conv2 and LN2, transparent SE: every trunk channel at six pixels, 8 at every pixel"""
    for off in tw.sigmas(C):
        sd, v0, v1 = tw.net_c(C, prec, off)
        ch, px = tw.conv_positions(C, off)
        with closing(engine_from_state(scamd, tmp_path, sd, 1, C, prec)) as eng:
            boards = tw.impulse_board(ch - off, px)
            x0, got = _debug(eng, boards, 0), _debug(eng, boards, 1)
        ref0, bd0 = tw.x0_impulse(len(ch), C, ch, px, v0[prec])
        _chunked(f"{C} {prec} (c) stem map +{off}, stage 0", x0, lambda s: (ref0[s], bd0[s]), len(ch))
        _chunked(f"{C} {prec} (c) stem map +{off}", got, lambda s: tw.form_c(sd, prec, 0, ch[s], px[s], v0[prec], v1[prec]), len(ch))


@pytest.mark.parametrize("C,prec", INST, ids=IDS)
def test_conv1_impulse(scamd, tmp_path, C, prec):
    """(d) pass-through stem, natural conv1 and LN1, identity conv2, natural LN2, transparent SE; rows with elements on a rounding tie
    are held to the nearest of their rounding variants"""
    for off in tw.sigmas(C):
        sd, v0 = tw.net_d(C, prec, off)
        ch, px = tw.conv_positions(C, off)
        with closing(engine_from_state(scamd, tmp_path, sd, 1, C, prec)) as eng:
            got = _debug(eng, tw.impulse_board(ch - off, px), 1)
        _chunked(f"{C} {prec} (d) stem map +{off}", got, lambda s: tw.form_d(sd, prec, 0, ch[s], px[s], v0[prec]), len(ch))


# ---------------------------------------------------------------------------------- e, f: exact sums
@pytest.mark.parametrize("C,prec", INST, ids=IDS)
def test_block_convs_exact_sums(scamd, tmp_path, C, prec):
    """(e) a constant stem output in front of a grid conv1 or conv2: the full 9 C / 16-step K loop at interior, edge and corner
    pixels; the probe removes the input, so 7 differing boards give the same bits"""
    boards = _dense(7)
    sd, kap, kap1 = tw.net_e2(C, prec)
    with closing(engine_from_state(scamd, tmp_path, sd, 1, C, prec)) as eng:
        got = _debug(eng, boards, 1)
    ref, bd = tw.form_e2(sd, 0, kap, kap1)
    tw.compare(f"{C} {prec} (e) conv2", got[:1], ref[None], bd[None])
    assert all(np.array_equal(bits_zero_folded(got[0]), bits_zero_folded(g)) for g in got)
    sd, kap = tw.net_e1(C, prec)
    with closing(engine_from_state(scamd, tmp_path, sd, 1, C, prec)) as eng:
        got = _debug(eng, boards, 1)
    ref, bd, keep, alts = tw.form_e1(sd, prec, 0, kap)
    tw.compare(f"{C} {prec} (e) conv1", got[:1], ref[None], bd[None], keep[None], alts)
    assert all(np.array_equal(bits_zero_folded(got[0]), bits_zero_folded(g)) for g in got)


@pytest.mark.parametrize("C,prec", INST, ids=IDS)
def test_squeeze_excitation_exact_sums(scamd, tmp_path, C, prec):
    """(f) LN2 a constant layer, SE weights on dyadic grids: the only inexact steps are __expf, rcp, one product and one add; scales
    near 1/2, moderate and saturated at both ends; every input and every pixel gives the same bits"""
    boards = _dense(5)
    for bname in tw.betas(C):
        sd, kap, beta = tw.net_f(C, prec, bname)
        with closing(engine_from_state(scamd, tmp_path, sd, 1, C, prec)) as eng:
            x0, got = _debug(eng, boards, 0), _debug(eng, boards, 1)
        assert np.array_equal(x0, np.broadcast_to(np.maximum(kap, 0), x0.shape))   # the constant stem, exactly
        ref, bd, _, z = tw.form_f(sd, 0, kap, beta)
        tw.compare(f"{C} {prec} (f) {bname} (z from {z.min():.1f} to {z.max():.1f})", got[0, :1], ref[None], bd[None])
        assert all(np.array_equal(bits_zero_folded(got[0, 0]), bits_zero_folded(r)) for g in got for r in g)


# ---------------------------------------------------------------------------------- g: block position and ring carry
@pytest.mark.parametrize("C,prec", INST, ids=IDS)
def test_block_position_and_ring_carry(scamd, tmp_path, C, prec):
    """(g) a 3-block net with form (c) in block k and the other two transparent, each block with weights of its own: stages before k
    are the stem's output bit for bit, stage k is the closed form, stages k..3 and the latent are bit-identical -- the weight ring is
    handed from conv to conv and from block to block, and wraps on the last block"""
    ch, px = tw.impulse_set([], range(112))
    boards = tw.impulse_board(ch, px)
    for k in range(3):
        sd, v0, v1 = tw.net_c(C, prec, 0, nb=3, blk=k)
        with closing(engine_from_state(scamd, tmp_path, sd, 3, C, prec)) as eng:
            st = {s: _debug(eng, boards, s) for s in (0, 1, 2, 3, 1000)}
        for s in range(1, k + 1):
            assert np.array_equal(bits_zero_folded(st[s]), bits_zero_folded(st[0])), (k, s)
        _chunked(f"{C} {prec} (g) block {k + 1} of 3", st[k + 1], lambda s: tw.form_c(sd, prec, k, ch[s], px[s], v0[prec], v1[prec]), len(ch))
        for s in list(range(k + 2, 4)) + [1000]:
            assert np.array_equal(bits_zero_folded(st[s]), bits_zero_folded(st[k + 1])), (k, s)
