"""GPU (-m gpu): every LayerNorm of the network -- stem, LN1, LN2, value head, both of the policy head -- on rows with a large common
offset, against the float64 TWO-PASS LayerNorm (tests/ln_offset_ref.py), at the four instantiations of the tower.

The engine's LayerNorm is one pass, var = Q / C - mean^2, so it loses precision with the square of mean / sigma.  A row
x[c] = M + s d[c], exact in float32, reaches a LayerNorm as the bias of a conv with zero weights; mean / sigma climbs the rungs 0, 8,
64, 512, 4096, 32768 with both signs of M, the 64 and 512 rungs repeat at s = 2^-8 and 2^8, and the 8, 64 and 512 rungs with d off
the 1/4 grid (the float32 sums of the row then round from the first rung on).  Three sites are read in fp32 (stage
0, stage 1, the log-probabilities), three through the operand rounding that follows them (LN1, the value head's feature row, the
policy head's first LayerNorm).  On every rung the device is finite and within the one-pass fp32 bound (assertion 1: a kernel that
loses more than its formula must lose fails).  On every rung up to R_REQ it is held to the operation itself (assertion 2: the error
is invisible next to the operand rounding that follows, or the operand IS the rounding of the exact value).  Above R_REQ the
measured error is printed beside the exact value, and the first rung that fails assertion 2 must be the one ln_offset_ref.ENVELOPE
records.  tests/test_tower_ref.py and tests/test_heads_ref.py hold the oracle to both assertions on every rung, show that a one-pass
fp32 LayerNorm in numpy fails assertion 2 above its break rung, and check the probes' conditions.

Every comparison prints its measured maximum, its bound or tolerance and the share of it that was used."""
from contextlib import closing

import numpy as np
import pytest

import ln_offset_ref as lo
import tower_ref as tw
from support import IDS, INST, engine_from_state, scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu


def _observed(eng, net):
    """-> {"stage", "logp", "value"}: the one row that every pixel of every position shows (asserted), the values per meta row"""
    boards = net.boards()
    assert len(boards) <= eng.L.sc_engine_max_batch(eng.h)
    stage = eng.debug(boards, np.zeros((len(boards), 7), np.int32), net.nb)
    logp, v = eng.forward(boards, net.meta)
    return {"stage": lo.one_row(stage, "stage"), "logp": lo.one_row(logp, "logp"), "value": lo.one_row(v, "value")}


@pytest.mark.parametrize("C,prec", INST, ids=IDS)
@pytest.mark.parametrize("kind", list(lo.NETS))
def test_layernorm_rows_with_a_common_offset(scamd, tmp_path, kind, C, prec):
    """net "s": stem LN and policy LN1; net "a": LN1; net "b": LN2, the 73-wide policy LN and the value LN -- 25 rows each, one
    engine a row"""
    tw.representable(lo.base(0 if kind == "s" else 1, C, prec, kind), prec)
    shares = {s: {} for s in lo.NETS[kind]}
    for r in lo.rows():
        net = lo.Net(kind, C, prec, r)
        with closing(engine_from_state(scamd, tmp_path, net.sd, net.nb, C, prec, skip=net.skip + net.unchanged)) as eng:
            got = _observed(eng, net)
        for st in net.sites:
            err1, big1, bd1 = st.check1(got[st.kind])
            sh2, err2, top, excused = st.check2(got[st.kind])
            print(f"{st.label()}: max |device - exact| {err2:.3e} (largest |exact| {top:.3e}); one-pass bound up to {bd1:.3e}, share used "
                  f"{err1:.3f}; share of assertion 2's tolerance {sh2:.3g}{f', {excused} elements on a tie tried both ways' if excused else ''}"
                  f"{'' if r[0] <= lo.R_REQ else ' (above R_REQ: recorded)'}")
            assert err1 <= 1.0, (st.label(), "beyond the one-pass bound", err1, big1)
            assert r[0] > lo.R_REQ or sh2 <= 1.0, (st.label(), "not the two-pass LayerNorm within the envelope", sh2, err2)
            shares[st.name][r] = sh2
    for s, sh in shares.items():
        env = lo.first_failing(sh)
        print(f"{C} {prec} {s}: first rung that fails assertion 2: {env} (recorded {lo.ENVELOPE[s, C, prec]}, required {lo.R_REQ}); "
              f"largest share of its tolerance up to R_REQ {max(v for r, v in sh.items() if r[0] <= lo.R_REQ):.3g}")
        assert env == lo.ENVELOPE[s, C, prec], (s, C, prec, env)
        assert env is None or env > lo.R_REQ
