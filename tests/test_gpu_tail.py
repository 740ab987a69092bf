"""GPU (-m gpu): the network's output tail against closed forms -- log-softmax over 4672 actions, legal-move priors, value tail.

The tail ends the tower in `k_tower32` and in the fused `k_step` and is the only float arithmetic whose results go straight into the
search tree.  Probe weights (tests/tail_ref.py) make its input known exactly whatever the trunk computes: a zero gain in the policy
head's last LayerNorm leaves the logit of move plane ch at the bias b[ch], zero feature columns in value_head.ffn.0 leave the value a
function of meta alone.  The reference is float64 arithmetic on the weights, the bounds are a handful of float32 roundings
(tail_ref.logp_bound / prior_bound / value_bound; tests/test_tail_ref.py holds the CPU oracle to the same bounds).  Engines have one
residual block (depth is irrelevant to the tail) and are built from weight blobs, in the four instantiations of the tower.

Every comparison prints its measured maximum beside its bound."""
import os
from contextlib import closing

import numpy as np
import pytest

import scw
import tail_ref as tr
from helpers import GpuPredictEvaluator, _assert_same, bits
from lines import WIDE, WIDE137
from support import GOLD, IDS, INST, scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu
SEED = 17


def _inputs(n):
    """n rows: four golden positions and an all-zero board, cycled"""
    g = np.load(os.path.join(GOLD, "nn_ref_b1_c256.npz"))
    boards = np.concatenate([g["boards"][[0, 3, 5, 7]], np.zeros((1, 8, 8, 112), np.int8)])
    meta = np.concatenate([g["meta"][[0, 3, 5, 7]], np.zeros((1, 7), np.int32)])
    r = np.arange(n) % 5
    return boards[r], meta[r]


def _engine(scamd, tmp_path, Cw, precision, b=None, vp=None, gain=None):
    """a one-block engine from a blob: seed-init weights with the policy probe b, the value probe vp, or the last policy gain x gain"""
    sd = scw.prng_state_dict(1, Cw, SEED)
    if b is not None:
        tr.policy_probe(sd, b)
    if vp is not None:
        tr.value_probe(sd, *tr.value_probes()[vp])
    if gain is not None:
        sd["policy_head.model.3.weight"] = sd["policy_head.model.3.weight"] * np.float32(gain)
    path = str(tmp_path / "w.scw")
    scw.write_scw(path, sd, 1, Cw)
    eng = scamd.Engine(weights=path, precision=precision)
    assert eng.precision == precision
    return eng


# ---------------------------------------------------------------------------------- a. log-softmax
@pytest.mark.parametrize("Cw,precision", INST, ids=IDS)
def test_log_softmax_equals_the_closed_form(scamd, tmp_path, Cw, precision):
    """every bias pattern: logp within tail_ref.logp_bound of b[ch] - log(64 sum exp b); rows of different inputs and the 64 actions of
    a plane bit-identical; `low` (levels - 64) against `levels` within the bound (the max subtraction)"""
    boards, meta = _inputs(5)
    got = {}
    for name, b in tr.bias_patterns().items():
        with closing(_engine(scamd, tmp_path, Cw, precision, b=b)) as eng:
            lp, _ = eng.forward(boards, meta)
        ref, bd = tr.logp_closed(b), tr.logp_bound(b)
        near = np.abs(ref) <= 40
        assert bd[near].max() < tr.CEIL_LOGP
        err = np.abs(lp[0].astype(np.float64) - ref)
        print(f"{Cw} {precision} {name}: max |logp - closed form| {err.max():.2e} (bound {bd[np.argmax(err)]:.2e}; largest share of the "
              f"bound {(err / bd).max():.3f}; bound at |logp| <= 40: {bd[near].max():.2e})")
        assert np.isfinite(lp).all() and (err <= bd).all(), (name, err.max(), bd[np.argmax(err / bd)])
        assert all(np.array_equal(bits(r), bits(lp[0])) for r in lp), name                  # the probe removes the input
        assert np.array_equal(bits(lp[0]).reshape(73, 64), np.repeat(bits(lp[0])[::64], 64).reshape(73, 64)), name
        got[name] = lp[0].astype(np.float64)
    d = np.abs(got["low"] - got["levels"])
    bd = tr.logp_bound(tr.bias_patterns()["low"]) + tr.logp_bound(tr.bias_patterns()["levels"])
    print(f"{Cw} {precision}: max |logp(low) - logp(levels)| {d.max():.2e} (bound {bd[np.argmax(d)]:.2e})")
    assert (d <= bd).all()


# ---------------------------------------------------------------------------------- b. priors
def _prior_rows(logp_rows, rng):
    """[(row, width, set name, idx)]: every width x index set on a row of its own, an n_legal = 0 row behind each"""
    rows, r = [], 0
    for n in tr.WIDTHS:
        for sname, idx in tr.index_sets(logp_rows[r % len(logp_rows)], n, rng).items():
            rows.append((r, n, sname, np.asarray(idx, np.int64)))
            r += 2
    return rows, r


def _check_priors(eng, label, rows, n_rows, logp_of_row, arg_err_of_row):
    boards, meta = _inputs(n_rows)
    legal = [np.zeros(0, np.uint16)] * n_rows
    for r, _, _, idx in rows:
        legal[r] = idx.astype(np.uint16)
    pri, val = eng.predict(boards, meta, legal)
    _, val_f = eng.forward(boards, meta, want_logp=False)
    assert np.array_equal(bits(val), bits(val_f)), label                  # empty rows between the others change no value
    assert all(len(pri[r]) == 0 for r in range(1, n_rows, 2))
    worst = dict(rel=0.0, bound=0.0, share=0.0, gap=0.0, gap_bound=0.0)
    for r, n, sname, idx in rows:
        lp = logp_of_row(r)
        ref = tr.priors_from_logp(lp, idx)
        bd, rel = tr.prior_bound(lp, idx, arg_err_of_row(r, idx))
        assert rel.max() < tr.CEIL_PRIOR, (label, n, sname)
        p = pri[r].astype(np.float64)
        err = np.abs(p - ref)
        assert len(p) == n and np.isfinite(p).all() and (err <= bd).all(), (label, n, sname, int(np.argmax(err / bd)), err.max())
        big = ref > 1e-30
        if big.any():
            k = int(np.argmax(np.where(big, err / np.where(big, ref, 1), 0)))
            if err[k] / ref[k] > worst["rel"]:
                worst.update(rel=err[k] / ref[k], bound=rel[k])
        worst["share"] = max(worst["share"], float((err / bd).max()))
        # 1 - sum is the share the epsilon takes: exact value eps / (sum exp + eps)
        gap, gap_ref = 1.0 - p.sum(), 1.0 - ref.sum()
        assert p.sum() <= 1.0 and abs(gap - gap_ref) <= bd.sum(), (label, n, sname, gap, gap_ref)
        if abs(gap - gap_ref) > worst["gap"]:
            worst.update(gap=abs(gap - gap_ref), gap_bound=bd.sum())
    print(f"{label}: max rel prior error {worst['rel']:.2e} (bound {worst['bound']:.2e}; largest share of a bound {worst['share']:.3f}); "
          f"max |(1 - sum) - exact| {worst['gap']:.2e} (bound {worst['gap_bound']:.2e})")


@pytest.mark.parametrize("Cw,precision", INST, ids=IDS)
def test_priors_at_every_lane_round_width_probe_nets(scamd, tmp_path, Cw, precision):
    """widths 1..218 x (random, top n, bottom n, arg-max + arg-min) on every bias pattern, one `predict` per net, against
    priors_from_logp of the closed form; the bottom sets of `levels` and `far` hold far less mass than 1e-5, so their priors are
    e / 1e-5: a wrong or missing epsilon shows at once"""
    for name, b in tr.bias_patterns().items():
        ref, bd = tr.logp_closed(b), tr.logp_bound(b)
        rows, n_rows = _prior_rows([ref], np.random.default_rng(3))
        if name in ("levels", "far"):
            assert all(np.exp(ref[idx]).sum() < 1e-8 for _, n, s, idx in rows if s == "bottom")
        with closing(_engine(scamd, tmp_path, Cw, precision, b=b)) as eng:
            _check_priors(eng, f"{Cw} {precision} {name}", rows, n_rows, lambda r: ref, lambda r, idx: bd[idx])


@pytest.mark.parametrize("Cw,precision", INST, ids=IDS)
def test_priors_at_every_lane_round_width_natural_nets(scamd, tmp_path, Cw, precision):
    """the same widths and index sets on seed-init weights and on seed-init weights with the last policy gain x 8 (log-probabilities
    below -30), against priors_from_logp of the engine's own `forward` logp: that float is the kernel's s_z - lse, the argument of
    the prior's exponential"""
    for label, gain in (("plain", None), ("sharp", 8.0)):
        with closing(_engine(scamd, tmp_path, Cw, precision, gain=gain)) as eng:
            lp5, _ = eng.forward(*_inputs(5))
            if gain is not None:
                assert lp5.min() < -30, lp5.min()      # else raise the gain
            rows, n_rows = _prior_rows(lp5, np.random.default_rng(4))
            lp, _ = eng.forward(*_inputs(n_rows))
            assert np.array_equal(bits(lp[:5]), bits(lp5))
            _check_priors(eng, f"{Cw} {precision} {label} (min logp {lp.min():.1f})", rows, n_rows, lambda r: lp[r], lambda r, idx: 0.0)


# ---------------------------------------------------------------------------------- c. argmax
@pytest.mark.parametrize("Cw,precision", INST, ids=IDS)
def test_argmax_branch_on_exact_ties(scamd, tmp_path, Cw, precision):
    """predict(argmax=True) on probe nets: several actions of the maximal plane (exact ties) sit on both sides of every lane-round
    boundary of the width; the one-hot is at the LAST of them (src/chess.rs:880-889) and the value is that of the plain call"""
    rng = np.random.default_rng(6)
    for name in ("levels", "wave1", "far"):
        b = tr.bias_patterns()[name]
        top = int(np.argmax(b))
        assert np.sum(b == b.max()) == 1
        others = np.setdiff1d(np.arange(4672), np.arange(top * 64, top * 64 + 64))
        legal, want = [], []
        for n in (65, 129, 193, 218):
            at = [0] + [p for bd in (64, 128, 192) if bd < n for p in (bd - 1, bd)]
            for pos in (at, at[:-1]):                   # the last tie just behind the last boundary, then just in front of it
                idx = rng.permutation(others)[:n]
                idx[pos] = top * 64 + rng.permutation(64)[:len(pos)]
                legal.append(idx.astype(np.uint16))
                want.append(pos[-1])
        boards, meta = _inputs(len(legal))
        with closing(_engine(scamd, tmp_path, Cw, precision, b=b)) as eng:
            pri, val = eng.predict(boards, meta, legal)
            hot, val_a = eng.predict(boards, meta, legal, argmax=True)
        assert np.array_equal(bits(val), bits(val_a)), name
        for p, h, idx, w in zip(pri, hot, legal, want):
            ties = np.flatnonzero(idx // 64 == top)
            assert ties[-1] == w and len(set(bits(p[ties]))) == 1 and (p[ties] > np.delete(p, ties).max()).all(), (name, len(idx))
            assert np.array_equal(h, np.eye(len(idx), dtype=np.float32)[w]), (name, len(idx), int(np.argmax(h)), w)
    print(f"{Cw} {precision}: one-hot at the last of the tied maxima at widths 65, 129, 193, 218")


# ---------------------------------------------------------------------------------- d. value
@pytest.mark.parametrize("Cw,precision", INST, ids=IDS)
def test_value_equals_the_closed_form(scamd, tmp_path, Cw, precision):
    """130 rows of the meta grid (turn, fullmove 1..1023, halfmove 0..149, castling bits) in one batch -- the 64-row tiles of
    k_value_fc1 are crossed at 64/65 and at 128 -- on a probe whose tanh argument covers (-2.8, 2.8) and on a saturated one; the same
    rows give the same bits in batches of 1, 64, 65 and 130"""
    grid = tr.meta_grid()
    boards, _ = _inputs(len(grid))
    for vname, p in tr.value_probes().items():
        with closing(_engine(scamd, tmp_path, Cw, precision, vp=vname)) as eng:
            _, v = eng.forward(boards, grid, want_logp=False)
            ref, bd = tr.value_closed(grid, *p), tr.value_bound(grid, *p)
            err = np.abs(v.astype(np.float64) - ref)
            print(f"{Cw} {precision} {vname}: max |value - closed form| {err.max():.2e} (bound {bd[np.argmax(err)]:.2e}; largest share of "
                  f"the bound {(err / bd).max():.3f})")
            assert np.isfinite(v).all() and (err <= bd).all(), (vname, grid[np.argmax(err / bd)], err.max())
            if vname == "saturated":
                assert (np.abs(np.abs(v) - 1) <= 2.0 ** -23).all() and np.array_equal(np.sign(v), 2.0 * grid[:, 0] - 1)
            for n in (1, 64, 65):
                _, vn = eng.forward(boards[:n], grid[:n], want_logp=False)
                assert np.array_equal(bits(vn), bits(v[:n])), (vname, n)
            _, v2 = eng.predict(boards, grid, [np.arange(3, dtype=np.uint16)] * len(grid))
            assert np.array_equal(bits(v2), bits(v)), vname


# ---------------------------------------------------------------------------------- e. the search's copy of the tail
def _roots(orc):
    """(name, line, fen, oracle state): 20, 82, 137 and 218 legal moves"""
    out = []
    for name, line, fen, width in (("start", [], None, 20), ("wide82", WIDE, None, 82), ("wide137", WIDE137, None, 137),
                                   ("fen218", [], tr.FEN218 % (98, 303), 218)):
        st = orc.State(fen)
        for m in line:
            st.push(m)
        assert len(st.legal_moves()) == width and st.outcome() is None
        out.append((name, line, fen, st))
    return out


@pytest.mark.parametrize("n_slots", [64, 1], ids=["one_launch", "two_launches"])
@pytest.mark.parametrize("Cw,precision", INST, ids=IDS)
def test_search_copy_of_the_tail(scamd, orc, tmp_path, Cw, precision, n_slots):
    """SelfPlay on a probe engine (`levels` + `spread`), fused step (64 slots) and two-launch form (1 slot): after one simulation the
    root's priors are `predict`'s bit for bit and within the prior bound of the closed form on the oracle's action indices, and the
    backed-up value is within the value bound of value_closed(meta) (the 218 root has fullmove 303: 304 as bfloat16).  Then 60
    simulations from the 218 root in lockstep with the oracle search fed the engine's `predict`: the first network-prior root of
    four lane rounds"""
    b, vp = tr.bias_patterns()["levels"], tr.value_probes()["spread"]
    lp_ref, lp_bd = tr.logp_closed(b), tr.logp_bound(b)
    eng = _engine(scamd, tmp_path, Cw, precision, b=b, vp="spread")
    opened = [eng]                              # closed whatever happens: an open handle keeps the one-launch form to itself
    try:
        roots = _roots(orc)
        slots = [0, 17, 40, 63] if n_slots == 64 else [0, 0, 0, 0]
        kw = dict(n_slots=n_slots, n_games=n_slots, rollout_num=100, num_steps=4, cpuct=2.5, with_noise=False, seed=5)
        sp = None
        if n_slots == 64:
            sp = scamd.SelfPlay(eng, **kw)
            opened.append(sp)
            assert sp.launches_per_step() == 1      # whole 64-slot block: the fused step
            for slot, (name, line, fen, st) in zip(slots, roots):
                sp.set_position(slot, line, fen=fen)
            sp.enqueue(1)
            sp.sync()
        for slot, (name, line, fen, st) in zip(slots, roots):
            h = sp
            if n_slots == 1:                        # one handle per root, one at a time: k_step + k_value_fc1
                h = scamd.SelfPlay(eng, **kw)
                opened.append(h)
                assert h.launches_per_step() == 2
                h.set_position(slot, line, fen=fen)
                h.enqueue(1)
                h.sync()
            srch, ev = orc.Search(st), GpuPredictEvaluator(orc, eng)
            srch.sim(evaluator=ev.fn, cpuct=2.5, with_noise=False)
            t = h.tree(slot)
            n = len(st.legal_moves())
            _assert_same(t, srch.dump(), ev, name)
            assert t["n_child"][0] == n and np.array_equal(bits(t["prior"][1:1 + n]), bits(ev.priors[0])), name
            idx = np.asarray([orc.move_index(m, st.turn) for m in st.legal_moves()], np.int64)
            ref = tr.priors_from_logp(lp_ref, idx)
            bd, rel = tr.prior_bound(lp_ref, idx, lp_bd[idx])
            err = np.abs(t["prior"][1:1 + n].astype(np.float64) - ref)
            meta = st.encode()[1]
            v_ref, v_bd = tr.value_closed(meta, *vp)[0], tr.value_bound(meta, *vp)[0]
            v_err = abs(float(t["q"][0]) - v_ref)
            print(f"{Cw} {precision} {n_slots} slots {name}: max rel prior error {(err / ref).max():.2e} (bound {rel.max():.2e}); "
                  f"|q[0] - closed form| {v_err:.2e} (bound {v_bd:.2e})")
            assert (err <= bd).all() and rel.max() < tr.CEIL_PRIOR, name
            assert t["n"][0] == 1 and bits(t["q"][0]) == bits(ev.values[0]) and v_err <= v_bd, (name, t["q"][0], v_ref)
            if name == "fen218":
                assert meta[1] == 303 and tr.bf16_rne(np.float32(303)) == 304
                done = 1
                for burst in [1] * 9 + [2, 3, 5, 7] * 3:
                    h.enqueue(burst)
                    h.sync()
                    done += burst
                    for _ in range(burst):
                        srch.sim(evaluator=ev.fn, cpuct=2.5, with_noise=False)
                    _assert_same(h.tree(slot), srch.dump(), ev, (name, done))
                    assert list(h.slot(slot)["path"]) == list(srch.last_path()), (name, done)
                assert done == 61 and srch.dump()["n"][0] == 61
            assert h.stats()["error_flags"] == 0
            if n_slots == 1:
                h.close()
    finally:
        for h in reversed(opened):
            h.close()
