"""GPU (-m gpu): the end-of-ply move choice (mcts::step, src/mcts.rs:298-317; NNPlayer::bestmove, src/play.rs:268-277) of the
device against the host, on crafted inputs.

`sc_debug_choose_child` runs `choose_child` of csrc/search_expand.hpp -- the function `k_mcts` and the fused `k_step` call at
the end of every ply -- on given visit counts, one wave per case.  Every assertion is exact equality: the chosen index, and the
bit pattern of the f32 weight total.  The reference of a decision is the oracle's `orc_choose_child` (oracle/mcts.c), the
reference of a single weight is the host libm's `powf` through ctypes (what Rust's `f32::powf` and the oracle call); numpy's own
f32 power is no reference.  tests/test_oracle_mcts.py holds the oracle to a plain Python restatement on the same inputs."""
import numpy as np
import pytest

import choice_cases as cc
from helpers import GpuPredictEvaluator, bits
from support import scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32


def _assert_cases_equal_oracle(scamd, orc, cases, what):
    n_act, nc, temp, u = cc.pack(cases)
    want_c, want_t = cc.oracle_choices(orc, n_act, nc, temp, u)
    got_c, got_t = scamd.choose_child(n_act, nc, temp, u)
    bad = np.flatnonzero((got_c != want_c) | (bits(got_t) != bits(want_t)))
    for i in bad[:20]:
        print(f"{what}: case {i}: nc={nc[i]} T={temp[i]!r} u={u[i]!r} counts={n_act[i, :nc[i]].tolist()} device choice={got_c[i]} "
              f"total={got_t[i]!r} (0x{bits(got_t)[i]:08x}); oracle choice={want_c[i]} total={want_t[i]!r} (0x{bits(want_t)[i]:08x})")
    assert bad.size == 0, f"{what}: {bad.size} of {len(cases)} cases differ from the oracle (first: {bad[:10].tolist()})"
    return got_c, got_t


def test_weights_equal_host_powf(scamd, orc):
    """nc = 1: the total IS the weight.  Every count 0..1024 (rollouts 180, 300, 800 included) at every temperature of the
    grid: the device's weight has the bit pattern of libm powf((float)n, 1.0f / T), and of the oracle's total."""
    counts = np.arange(1025, dtype=np.int32)
    cases = [([int(n)], T, F(0.5)) for T in cc.TEMPS for n in counts]
    n_act, nc, temp, u = cc.pack(cases)
    want = np.array([cc.host_powf(F(n[0]), F(1.0) / F(T)) for n, T, _ in cases], np.float32)
    assert np.isfinite(want).all()
    orc_c, orc_t = cc.oracle_choices(orc, n_act, nc, temp, u)
    assert np.array_equal(bits(orc_t), bits(want)) and not orc_c.any()
    got_c, got_t = scamd.choose_child(n_act, nc, temp, u)
    bad = np.flatnonzero(bits(got_t) != bits(want))
    for i in bad[:40]:
        n, T = cases[i][0][0], cases[i][1]
        p = F(1.0) / F(T)
        print(f"count {n} power {p!r} (T={T}): device 0x{bits(got_t)[i]:08x} host 0x{bits(want)[i]:08x} "
              f"float64 {float(n) ** float(p)!r}")
    per_t = {T: int(sum(1 for i in bad if cases[i][1] == T)) for T in cc.TEMPS}
    assert bad.size == 0, f"{bad.size} of {len(cases)} weights differ from host powf; per temperature: {per_t}"
    assert not got_c.any()


def test_choice_next_to_every_kind_of_boundary(scamd, orc):
    """count vectors of every width (1 child .. 224, around the 64-lane rounds), rollout budget and shape, each at two
    temperatures of the grid (+ 1.0), with u = 0, 1 - 2^-24, uniform lattice draws and the lattice points on either side of
    cumulative boundaries: index and total equal the oracle's"""
    cases = cc.boundary_cases()
    assert 3000 < len(cases) < 20000
    assert {len(n) for n, _, _ in cases} == set(cc.NCS) and {t for _, t, _ in cases} == set(cc.TEMPS + [1.0])
    got_c, _ = _assert_cases_equal_oracle(scamd, orc, cases, "boundary")
    # the inputs do sit on boundaries: many cases are decided by an exact cum == x, and neighbours on the lattice differ
    assert len(set(got_c.tolist())) > 50


def _tie_vectors():
    """(counts, positions of the maxima): maxima at the lanes / rounds the reduction can get wrong, all-equal vectors, nc = 1"""
    out = []
    spots = [0, 63, 64, 65, 128, 223]
    for nc in cc.NCS:
        out.append(([7] * nc, list(range(nc))))
        inside = [s for s in spots if s < nc]
        for a in inside:
            for b in inside:
                if a <= b:
                    n = [(i * 7 + 3) % 5 for i in range(nc)]      # background 0..4, below the maxima
                    n[a] = n[b] = 9
                    out.append((n, sorted({a, b})))
        if len(inside) > 2:
            n = [(i * 5 + 1) % 4 for i in range(nc)]
            for s in inside:
                n[s] = 300
            out.append((n, inside))
    return out


def test_temperature_zero_first_maximum(scamd, orc):
    """temperature 0 (mcts.rs:309-311): the FIRST most-visited child, with the maxima in lanes 0/63, across the rounds
    (64/65/128/223), in one lane twice (0 and 64, 0 and 128), everywhere (all-equal) and nc = 1"""
    vecs = _tie_vectors()
    cases = [(n, 0.0, F(0.5)) for n, _ in vecs]
    got_c, got_t = _assert_cases_equal_oracle(scamd, orc, cases, "first maximum")
    assert got_c.tolist() == [mx[0] for _, mx in vecs]
    assert not bits(got_t).any()


def test_temperature_zero_random_among_the_maxima(scamd):
    """tie_random (play.rs:268-277): the floor(u * count)-th most-visited child in index order, against a plain restatement;
    u = 0, 1 - 2^-24, lattice draws and the lattice points around every k / count"""
    rnd = np.random.RandomState(3)
    cases, want = [], []
    for n, mx in _tie_vectors():
        us = [F(0.0), cc.U_LAST] + [cc.lattice_u(k) for k in rnd.randint(0, cc.LATTICE, 3)]
        js = set(range(1, len(mx))) if len(mx) <= 12 else {1, len(mx) - 1} | set(rnd.randint(1, len(mx), 10).tolist())
        for j in sorted(js):
            k0 = j * cc.LATTICE // len(mx)
            us += [cc.lattice_u(k0 + d) for d in (-1, 0, 1)]
        for u in sorted({float(x) for x in us}):
            cases.append((n, 0.0, F(u)))
            want.append(cc.choose_ref(n, 0.0, F(u), tie_random=True)[0])
    n_act, nc, temp, u = cc.pack(cases)
    got_c, got_t = scamd.choose_child(n_act, nc, temp, u, tie_random=True)
    bad = np.flatnonzero(got_c != np.array(want, np.int32))
    for i in bad[:20]:
        print(f"tie_random: nc={nc[i]} u={u[i]!r} counts={n_act[i, :nc[i]].tolist()} device {got_c[i]} want {want[i]}")
    assert bad.size == 0 and not bits(got_t).any()
    assert len(set(got_c.tolist())) > 6


def test_degenerate_totals_agree_with_the_oracle(scamd, orc):
    """RECORDED BEHAVIOUR, NOT REFERENCE PARITY.  With all counts zero (a rollout budget of 1 expands the root only) the total is
    0; at a temperature small enough for N^(1/T) to overflow f32 (T = 0.05, count 800) it is infinite, and u = 0 then makes
    x = NaN.  The reference panics on both in WeightedIndex::new(..).unwrap(); the oracle and the device quietly return an index.
    Pinned here: they return the SAME index and the same total bits (zero or infinite total: every cumulative sum is <= x, the
    last child; infinite total and u = 0: x is NaN, no comparison holds, child 0)."""
    cases = cc.degenerate_cases()
    got_c, got_t = _assert_cases_equal_oracle(scamd, orc, cases, "degenerate")
    tot = {float(t) for t in got_t}
    assert tot == {0.0, float("inf")}
    for (n, T, u), c, t in zip(cases, got_c, got_t):
        assert c == (0 if np.isinf(t) and u == 0 else len(n) - 1)


GAME_CFG = dict(rollout_num=20, num_steps=40, cpuct=2.5, temperature_switch=2, with_noise=False)


@pytest.mark.parametrize("temperature", [0.5, 2.0])
def test_selfplay_games_exact_at_fractional_temperature(scamd, orc, temperature):
    """whole games whose every ply after the second is SAMPLED at a fractional temperature == the oracle's traces (the
    comparison of test_selfplay_games_exact, which plays at temperature 0)"""
    cfg = dict(GAME_CFG, temperature=temperature)
    sp = scamd.SelfPlay(None, n_slots=8, n_games=16, evaluator="synth", seed=13, first_game_id=300, outcome_gate=100, **cfg)
    sp.run()
    st = sp.stats()
    assert st["games_finished"] == 16 and st["games_active"] == 0 and st["error_flags"] == 0
    for gi in range(16):
        tr = sp.trace(gi)
        ref = orc.selfplay_game(seed=13, game_id=tr["game_id"], outcome_gate=100, **cfg)
        assert tr["steps"] == ref["steps"], gi
        assert tr["outcome"] == ref["outcome"], gi
    sp.close()


def test_net_in_the_loop_games_exact_at_fractional_temperature(scamd, orc):
    """the same through the network and the fused one-launch step (k_step), at temperature 0.6: the oracle plays with the
    engine's `predict` as its evaluator (the pattern of test_net_in_the_loop_games_exact)"""
    cfg = dict(rollout_num=40, num_steps=7, cpuct=2.5, temperature=0.6, temperature_switch=2, with_noise=False)
    eng = scamd.Engine(2, 128, seed=22, precision="bf16")
    sp = scamd.SelfPlay(eng, n_slots=64, n_games=64, seed=9, first_game_id=700, outcome_gate=100, **cfg)
    assert sp.launches_per_step() == 1
    sp.run()
    assert sp.stats()["error_flags"] == 0 and sp.stats()["games_finished"] == 64
    for g in (0, 21, 63):
        tr = sp.trace(g)
        ev = GpuPredictEvaluator(orc, eng)
        ref = orc.selfplay_game(evaluator=ev.fn, seed=9, game_id=tr["game_id"], outcome_gate=100, **cfg)
        assert len(ev.values) > 200
        assert tr["steps"] == ref["steps"] and tr["outcome"] == ref["outcome"], g
    sp.close()
    eng.close()
