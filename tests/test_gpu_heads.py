"""GPU (-m gpu): the heads of the network -- value conv, its LayerNorm + ReLU, the bf16 feature row and the FC1 packing that must match
its order, the split-K FC1 GEMM, policy conv1, its LayerNorm without ReLU, policy conv2, the 73-wide LayerNorm and the channel-major
flatten -- against float64 closed forms on probe weights (tests/heads_ref.py), at the four instantiations of the tower.

The heads have no debug output, so they are checked end to end through `forward`: sign-pattern LayerNorms make the operand of every
head conv known exactly (+-g, or g / 0 behind a ReLU), every sum up to the FC1 output h[128] and the conv2 output is exact in fp32 in
any order, and what is left is the last LayerNorm, the log-softmax and the value tail, each with a bound of a handful of float32
roundings counted from the code.  A feature column packed to the wrong (channel, pixel), two pixels exchanged, a stale row in a
64-position tile, a fragment read from the wrong slot or a padded policy channel in the LayerNorm sums moves a result by hundreds of
bounds.  tests/test_heads_ref.py holds the CPU oracle to the same closed forms, asserts the probes' conditions on these very position
sets and shows that six subtly wrong nets fail.  Engines are built from weight blobs, one per probe net.

Every comparison prints its measured maximum, the bound at that element and the largest share of a bound that was used."""
from contextlib import closing

import numpy as np
import pytest

import heads_ref as hr
import tower_ref as tw
from helpers import bits, golden_boards
from support import IDS, INST, engine_from_state, scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu


def _value_set():
    """every plane x every pixel as a lone impulse (7168 rows), the dense set of the trunk tests, six multi-impulse boards"""
    b = np.concatenate([hr.impulse_positions(), tw.dense_boards(golden_boards()), hr.random_boards(6)])
    return b, hr.metas(len(b))


def _policy_set():
    """16 multi-impulse boards (every pixel a pattern of its own), the dense set, four lone impulses"""
    imp = hr.impulse_positions()
    return np.concatenate([hr.random_boards(16), tw.dense_boards(golden_boards()), imp[[0, 1000, 3333, 7167]]])


def _values(eng, boards, meta, size=2048):
    out = np.concatenate([eng.forward(boards[s], meta[s], want_logp=False)[1] for s in tw.chunks(len(boards), size)])
    assert np.isfinite(out).all()
    return out


def _batch_edges(label, eng, boards, meta, big_v=None, big_lp=None):
    """batches of 1, 63, 64, 65 and 129 rows, distinct rows in each, from different places of the large batch: the same bits as there
    (the 64-position FC1 tiles, the n_pos masking, rows that change their place in a tile)"""
    n = len(boards)
    for size, start in zip(hr.BATCHES, (5, n // 7, n // 3, n // 2 + 11, n - 129)):
        s = slice(start, start + size)
        assert s.stop <= n
        lp, v = eng.forward(boards[s], meta[s], want_logp=big_lp is not None)
        if big_v is not None:
            assert np.array_equal(bits(v), bits(big_v[s])), (label, size)
        if big_lp is not None:
            assert np.array_equal(bits(lp), bits(big_lp[s])), (label, size)


# ---------------------------------------------------------------------------------- the latent the heads start from
@pytest.mark.parametrize("C,prec", INST, ids=IDS)
def test_latent_is_the_sign_pattern(scamd, tmp_path, C, prec):
    """the residual stream after the stem and at the end of a one-block net, rounded as the head convs round it, is G[c] [sign +] bit
    for bit, on lone impulses, dense and multi-impulse boards, for every probe net"""
    imp = hr.impulse_positions()
    boards = np.concatenate([imp[::61], tw.dense_boards(golden_boards()), hr.random_boards(4)])
    for k in range(len(hr.nets(C))):
        sd = hr.net(C, prec, k)
        want = hr.latent_form(sd, C, prec, boards)
        with closing(engine_from_state(scamd, tmp_path, sd, 1, C, prec)) as eng:
            for stage in (0, 1000):
                x = eng.debug(boards, np.zeros((len(boards), 7), np.int32), stage)
                assert np.isfinite(x).all()
                got = tw.r_act(x, prec)
                assert np.array_equal(bits(got + 0.0), bits(want)), (k, stage, int((got != want).sum()))
                gap = np.abs(x - want).max()
                print(f"{C} {prec} net {k} stage {stage}: latent operand equals the pattern; max |fp32 stream - pattern| {gap:.2e}")


# ---------------------------------------------------------------------------------- (v) the value head end to end
@pytest.mark.parametrize("C,prec", INST, ids=IDS)
def test_value_head(scamd, tmp_path, C, prec):
    """(v) value conv, LayerNorm + ReLU, feature order, FC1 packing, split-K GEMM, tail: every plane x pixel impulse, dense and
    multi-impulse boards, both values of meta[0], on every probe net; then the batch edges"""
    boards, meta = _value_set()
    top = 0.0
    for k in range(len(hr.nets(C))):
        sd = hr.net(C, prec, k)
        ref, bd, _ = hr.form_v(sd, C, prec, boards, meta)
        with closing(engine_from_state(scamd, tmp_path, sd, 1, C, prec)) as eng:
            v = _values(eng, boards, meta)
            top = max(top, tw.compare(f"{C} {prec} (v) net {k}, {len(boards)} positions", v, ref, bd))
            assert np.array_equal(np.sign(v), np.sign(ref))
            _batch_edges(f"(v) net {k}", eng, boards, meta, big_v=v)
    print(f"{C} {prec} (v): largest share of a bound {top:.3f}")


# ---------------------------------------------------------------------------------- (p) the policy head end to end
@pytest.mark.parametrize("C,prec", INST, ids=IDS)
def test_policy_head(scamd, tmp_path, C, prec):
    """(p) policy conv1, LayerNorm without ReLU, conv2, the 73-wide LayerNorm, flatten, log-softmax: all 4672 actions of multi-impulse
    boards whose pixels all differ, on every probe net and on the one with a large plane 72 (padded channels add nothing to the
    LayerNorm sums); then the batch edges"""
    boards = _policy_set()
    meta = hr.metas(len(boards))
    top = 0.0
    for k, big72 in [(k, False) for k in range(len(hr.nets(C)))] + [(0, True)]:
        sd = hr.net(C, prec, k, big72=big72)
        ref, bd = hr.form_p(sd, C, prec, boards)
        with closing(engine_from_state(scamd, tmp_path, sd, 1, C, prec)) as eng:
            lp, _ = eng.forward(boards, meta)
            top = max(top, tw.compare(f"{C} {prec} (p) net {k}{' big72' if big72 else ''}", lp, ref, bd))
            one, _ = eng.forward(boards[3:4], meta[3:4])
            assert np.array_equal(bits(one), bits(lp[3:4]))
            wide = np.concatenate([boards] * 5)[:129]
            lpw, _ = eng.forward(wide, hr.metas(129))
            assert np.array_equal(bits(lpw), bits(np.concatenate([lp] * 5)[:129])), k
    print(f"{C} {prec} (p): largest share of a bound {top:.3f}")


# ---------------------------------------------------------------------------------- (r) position in the tower
@pytest.mark.parametrize("C,prec", INST, ids=IDS)
def test_heads_at_every_depth(scamd, tmp_path, C, prec):
    """(r) forms (v) and (p) straight behind the stem (no block), behind one and behind three transparent blocks (head_conv0 = 1 + 2 nb
    moves the scale and ring indices the heads start from): the closed forms, and the same bits at the three depths"""
    imp = hr.impulse_positions()
    boards = np.concatenate([imp[::89], _policy_set()])
    meta = hr.metas(len(boards))
    got = {}
    for nb in (0, 1, 3):
        sd = hr.net(C, prec, 1, nb=nb)
        with closing(engine_from_state(scamd, tmp_path, sd, nb, C, prec)) as eng:
            got[nb] = eng.forward(boards, meta)
        assert np.isfinite(got[nb][0]).all() and np.isfinite(got[nb][1]).all()
        ref, bd, _ = hr.form_v(sd, C, prec, boards, meta)
        tw.compare(f"{C} {prec} (r) value, {nb} blocks", got[nb][1], ref, bd)
        ref, bd = hr.form_p(sd, C, prec, boards)
        tw.compare(f"{C} {prec} (r) logp, {nb} blocks", got[nb][0], ref, bd)
    for nb in (1, 3):
        assert np.array_equal(bits(got[nb][0]), bits(got[0][0])) and np.array_equal(bits(got[nb][1]), bits(got[0][1])), nb
