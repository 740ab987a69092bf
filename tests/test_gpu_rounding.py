"""GPU (-m gpu): how the device converts an fp32 activation into a matrix operand, at every conversion site of the network and at the
four instantiations of the tower: probe nets (tests/rounding_ref.py) put float32 values that sit ON the decision points of the operand
format -- every e4m3 midpoint with its two float32 neighbours, the subnormal ones included, the values that the clamp to 448 decides,
all 128 mantissa midpoints of three bf16 binades, zeros, negatives in front of a ReLU, both signs at the one signed site -- in front of
the site, and the result is held to the float64 closed forms of the trunk, head and tail tests evaluated at the operand that the stated
rule gives (nearest, ties to even, subnormals kept, clamp first).  A wrong neighbour anywhere moves the output that shows it by more
than a hundred bounds (tests/test_tower_ref.py and tests/test_heads_ref.py assert that, hold the CPU oracle to the same forms and show
that forms built from five wrong rules fail).  No bound is new.  The probes remove the input: every position gives the same bits.

Every case prints its decision points, the largest share of a bound that was used, and the rows held to a variant or left out."""
from contextlib import closing

import numpy as np
import pytest

import rounding_ref as rr
import tower_ref as tw
from helpers import golden_boards
from support import IDS, INST, engine_from_state, scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu


def _folded(a):
    """the bits of a float32 array with -0 read as +0 (ReLU is one v_max_f32, which may keep the sign of a zero)"""
    return (np.ascontiguousarray(a, np.float32) + np.float32(0)).view(np.uint32)


def _boards():
    """7 differing inputs: six dense boards, the all-ones board and the all-zero board among them"""
    b = tw.dense_boards(golden_boards())
    return b[[0, 1, 2, 3, 4, len(b) - 2, len(b) - 1]]


@pytest.mark.parametrize("C,prec", INST, ids=IDS)
@pytest.mark.parametrize("site", rr.SITES)
def test_operand_rounding_at_the_decision_points(scamd, tmp_path, site, C, prec):
    """site 1 stem -> conv1, 2 LN1 -> conv2, 3 block output -> next conv1, 4 policy LayerNorm -> policy conv2 (signed), 5 value
    LayerNorm -> bf16 features, 6p SE pool, 6h SE hidden vector (rounding_ref's module docstring)"""
    boards, zero_meta = _boards(), np.zeros((7, 7), np.int32)
    top, points, nets, held, left = 0.0, 0, 0, 0, 0
    for c in rr.cases(site, C, prec):
        if not nets:
            tw.representable(rr.base(c.nb, C, prec), prec)
        with closing(engine_from_state(scamd, tmp_path, c.sd, c.nb, C, prec, skip=c.skip)) as eng:
            if c.kind == "stage":
                if site == "3":          # block 1 hands relu(m / 2 + k0) = relu(x) to the probe block, bit for bit
                    assert np.array_equal(_folded(eng.debug(boards, zero_meta, 1)), _folded(np.broadcast_to(c.x, (7, 64, C)))), c.label()
                got = eng.debug(boards, zero_meta, c.nb)
                assert np.isfinite(got).all() and all(np.array_equal(_folded(got[0, 0]), _folded(r)) for g in got for r in g), c.label()
                got = got[:1, :1]
            elif c.kind == "logp":
                lp, _ = eng.forward(boards, c.meta)
                assert np.isfinite(lp).all() and all(np.array_equal(_folded(lp[0]), _folded(r)) for r in lp), c.label()
                got = lp[0]
            else:
                got = eng.forward(boards, c.meta, want_logp=False)[1]
                again = eng.forward(boards[::-1], c.meta, want_logp=False)[1]
                assert np.isfinite(got).all() and np.array_equal(_folded(got), _folded(again)), c.label()
        f = c.form()
        top = max(top, tw.compare(c.label(), got, *f))
        if len(f) == 4:
            held, left = held + len(f[3][0]), left + int(not f[2].all() and not len(f[3][0]))
        points, nets = points + int((~np.isnan(c.mid)).sum()), nets + 1
    print(f"{C} {prec} site {site} ({c.fmt} operands): {points} decision points in {nets} nets compared; largest share of a bound "
          f"{top:.3f}; rows held to a rounding variant {held}, left out {left} of {nets}")
    assert left == 0
