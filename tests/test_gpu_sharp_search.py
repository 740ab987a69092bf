"""GPU (-m gpu): the network inside the search loop on SHARP priors -- exact in the loop, bounded against the fp32 network.

Every other test that puts the network inside the search (tests/test_gpu_netloop.py, tests/test_gpu_deep_paths.py, the fp8 search
tests) uses seed-initialised weights, whose priors are nearly flat: the most visited root child gets a fifth of the visits and no
path is longer than 6 nodes.  A trained network is sharp, and there the search arithmetic works differently: priors span many
orders of magnitude, the U terms are tiny against Q, value backups run down long narrow lines, and one e4m3 rounding flip in a
logit is multiplied by the policy gain.  The networks are tests/sharp_nets.py's two recipes (g4v2: the trained-magnitude golden's;
g8: bench.py's sharp-prior run).

(a), (b): as in tests/test_gpu_netloop.py, the ORACLE's search driven by the engine's public `predict` must build the self-play
handle's tree bit for bit -- visit counts, value sums, uct words, priors, moves, paths; whole games move for move.
(c): the engine's search against the fp32 oracle network's recorded root visit counts (tests/golden/sharp_search_roots.json,
tools/gen_sharp_search_roots.py), in distribution, with bounds taken from the emulating oracles recorded beside them."""
import json
import os

import numpy as np
import pytest

import sharp_nets
from helpers import GpuPredictEvaluator, _assert_same
from lines import LINES, SLOTS
from support import GOLD, scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = [(10, 128, "bf16"), (10, 256, "bf16"), (10, 128, "fp8"), (3, 256, "fp8")]
LOCKSTEP = [(nb, C, p, kind, "one_launch") for nb, C, p in CASES for kind in sharp_nets.KINDS] + [(10, 128, "bf16", "g8", "separate_launches")]
SEED = 25   # the engine seed of (a): see test_sharp_lockstep_exact's docstring


@pytest.mark.parametrize("nb,C,precision,kind,form", LOCKSTEP, ids=[f"{nb}x{C}_{p}_{k}_{f}" for nb, C, p, k, f in LOCKSTEP])
def test_sharp_lockstep_exact(scamd, orc, tmp_path, nb, C, precision, kind, form):
    """120 simulations from the five LINES inside a 64-slot handle: each slot's node pool and last path equal the oracle search's
    that was fed the engine's own `predict` outputs, after every simulation for the first 24, then after bursts of 2, 3, 5, 7.
    The run must be in the sharp regime, judged on the ORACLE's tree: in at least three of the five slots the most visited root
    child holds >= 40 % of the root's visits at the end, and some compared path has >= 8 nodes.
    Engine seed 25 (21, the seed of tests/test_gpu_netloop.py, gives one slot of five at 10x256 g4v2; 22-24 pass with less room),
    checked beforehand on the CPU with the emulating oracle networks in the case's precision, the same searches and the same
    compared paths -- slots at >= 40 % / longest compared path:
      10x128 bf16  g4v2 4 / 10   g8 5 / 12        10x128 fp8  g4v2 4 / 10   g8 5 / 12
      10x256 bf16  g4v2 4 / 10   g8 5 / 10        3x256 fp8   g4v2 5 / 10   g8 5 / 10"""
    R = 120
    eng = sharp_nets.engine(scamd, tmp_path, nb, C, SEED, kind, precision)
    sp = scamd.SelfPlay(eng, n_slots=64, n_games=64, rollout_num=R + 20, num_steps=4, cpuct=2.5, with_noise=False, seed=5)
    assert sp.launches_per_step() == 1      # whole 64-slot block: the one-launch step
    if form == "separate_launches":
        sp.enable_timing(1)                 # every step timed: k_mcts, k_tower32 and k_value_fc1 as three launches
    searches, evs = [], []
    for slot, line in zip(SLOTS, LINES):
        sp.set_position(slot, line)
        st = orc.State()
        for m in line:
            st.push(m)
        searches.append(orc.Search(st))
        evs.append(GpuPredictEvaluator(orc, eng))
    done, longest, burst = 0, 0, [1] * 24 + [2, 3, 5, 7] * 40
    for b in burst:
        b = min(b, R - done)
        if b == 0:
            break
        sp.enqueue(b)
        sp.sync()
        done += b
        for slot, srch, ev in zip(SLOTS, searches, evs):
            for _ in range(b):
                srch.sim(evaluator=ev.fn, cpuct=2.5, with_noise=False)
            _assert_same(sp.tree(slot), srch.dump(), ev, (slot, done))
            path = list(srch.last_path())
            assert list(sp.slot(slot)["path"]) == path, (slot, done)
            longest = max(longest, len(path))
    assert done == R and sp.stats()["error_flags"] == 0
    shares = []
    for srch in searches:
        d = srch.dump()
        fc, nc = int(d["first_child"][0]), int(d["n_child"][0])
        assert d["n"][0] == R and d["n"][fc:fc + nc].sum() == R - 1
        shares.append(d["n"][fc:fc + nc].max() / (R - 1))
    print(f"{nb}x{C} {precision} {kind} {form}: share of the most visited root child per slot {np.round(shares, 2).tolist()}, longest compared path {longest}")
    assert sum(s >= 0.4 for s in shares) >= 3 and longest >= 8, (shares, longest)
    if form == "separate_launches":
        assert sp.timing(reset=False)["tower_launches"] >= R
    sp.close()
    eng.close()


@pytest.mark.parametrize("nb,C,precision", [(10, 128, "bf16"), (3, 256, "fp8")], ids=["10x128_bf16", "3x256_fp8"])
def test_sharp_games_exact(scamd, orc, tmp_path, nb, C, precision):
    """whole self-play games with the g8 network in the production form (ply transitions, temperature sampling in the first three
    plies, tree reset, the history planes of a growing line; nothing read between the launches): games 0, 21 and 63 of the 64
    equal the oracle's games played with the engine's `predict` as its evaluator: moves, root sums, children (N, Q, uct)"""
    cfg = dict(rollout_num=40, num_steps=7, cpuct=2.5, temperature=0.0, temperature_switch=3, with_noise=False)
    eng = sharp_nets.engine(scamd, tmp_path, nb, C, 22, "g8", precision)
    sp = scamd.SelfPlay(eng, n_slots=64, n_games=64, seed=9, first_game_id=500, outcome_gate=100, **cfg)
    assert sp.launches_per_step() == 1
    sp.run()
    assert sp.stats()["error_flags"] == 0 and sp.stats()["games_finished"] == 64
    for g in (0, 21, 63):
        tr = sp.trace(g)
        ev = GpuPredictEvaluator(orc, eng)
        ref = orc.selfplay_game(evaluator=ev.fn, seed=9, game_id=tr["game_id"], outcome_gate=100, **cfg)
        assert len(ev.values) > 100
        assert tr["steps"] == ref["steps"] and tr["outcome"] == ref["outcome"], g
    sp.close()
    eng.close()


# ---------------------------------------------------------------------------------- statistical, against the fp32 network
MULTIPLIER = 3   # of the emulating oracle's mean TVD: see test_sharp_search_statistics_against_the_fp32_oracle_network


def _tvd_and_agreement(ref, got):
    """(total-variation distances of the visit shares, number of rows where ref's most visited move is one of got's most visited)"""
    tv, agree = [], 0
    for a, b in zip(ref, got):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        tv.append(0.5 * np.abs(a / a.sum() - b / b.sum()).sum())
        agree += int(b[int(np.argmax(a))] == b.max())
    return np.asarray(tv), agree


@pytest.mark.parametrize("precision", ["bf16", "fp8"])
@pytest.mark.parametrize("kind", list(sharp_nets.KINDS))
def test_sharp_search_statistics_against_the_fp32_oracle_network(scamd, tmp_path, kind, precision):
    """The engine's search (6 x 128, seed 5, rollout 96, cpuct 2.5, no noise) with the bf16 / fp8 tower on the 48 fixture
    positions against the root visit counts of the oracle's search with the oracle's fp32 network on the same sharp weights:
    same move order, 95 visits, and in distribution (a 1-ulp prior change flips a near-tie and the trees diverge) the mean
    total-variation distance of the root visit shares and the share of positions where fp32's most visited move is one of the
    engine's most visited.

    The bounds are not the engine's own output.  The fixture also holds the counts of the oracle's bf16- and fp8-emulating
    networks: the engine's quantisation points, none of its code, a different summation order -- so the same distribution of
    deviations, not the same trees.  Bounds: mean TVD <= 3 x the emulating oracle's mean TVD for that kind and precision,
    agreement >= the emulating oracle's minus 3 of 48.  3 x, because one visit is 0.0105 of TVD, so a 48-position mean has a
    sampling error of about a third of the bf16 figure; at flat priors the engine's mean (0.0029) was about twice the emulating
    figure (0.0013 on 16 positions); and a systematic error in an operand map or a scale byte gives 0.1 and more at bf16.

    Emulating oracles against fp32 (from the fixture)     engine against fp32 (measured on an MI355X)
      g4v2 bf16  mean 0.0053  max 0.032  48/48            mean 0.0048  max 0.042  48/48
      g4v2 fp8   mean 0.0610  max 0.179  43/48            mean 0.0667  max 0.200  44/48
      g8   bf16  mean 0.0033  max 0.032  48/48            mean 0.0057  max 0.126  48/48
      g8   fp8   mean 0.0816  max 0.779  43/48            mean 0.1007  max 0.590  41/48
    (the engine's largest ratio to its emulating oracle is 1.7, g8 bf16: one position of the 48 diverged by 12 visits)"""
    with open(os.path.join(GOLD, "sharp_search_roots.json")) as fh:
        fx = json.load(fh)
    c, rows = fx["config"], fx["kinds"][kind]
    R = c["rollout"]
    assert (c["n_res_blocks"], c["channels"], c["seed"], R, c["cpuct"], c["with_noise"]) == (6, 128, 5, 96, 2.5, False) and len(rows) == 48
    emu_tv, emu_agree = _tvd_and_agreement([r["fp32"] for r in rows], [r[precision] for r in rows])
    eng = sharp_nets.engine(scamd, tmp_path, c["n_res_blocks"], c["channels"], c["seed"], kind, precision)
    counts = []
    for p in fx["positions"]:
        ge = scamd.search(eng, p["line"].split(), R, cpuct=c["cpuct"])[1]
        assert [ch[0] for ch in ge] == p["moves"].split(), p["line"]
        counts.append([int(ch[1]) for ch in ge])
        assert sum(counts[-1]) == R - 1, p["line"]
    eng.close()
    tv, agree = _tvd_and_agreement([r["fp32"] for r in rows], counts)
    print(f"{kind} {precision} engine vs fp32 oracle, 48 positions, rollout {R}: mean root visit TVD {tv.mean():.4f} (max {tv.max():.4f}), "
          f"arg-max-visit agreement {agree}/48; emulating oracle: mean {emu_tv.mean():.4f} (max {emu_tv.max():.4f}), {emu_agree}/48")
    assert tv.mean() <= MULTIPLIER * emu_tv.mean(), (tv.mean(), emu_tv.mean())
    assert agree >= emu_agree - 3, (agree, emu_agree)
