"""GPU (-m gpu): the network INSIDE the search loop, checked against something other than the engine itself.

The reference's search consumes `Game::predict` at every node (src/mcts.rs:149-152, src/backends/torch.rs:89-146).  In
self-play the engine produces those numbers on a path of its own: planes encoded straight into LDS by the helper wave of
`k_step`, the tower, `value_head.ffn.0` tiles computed inside the launch from rows handed over between workgroups
(`fc1_tail`), and the value tail (`value_tail_finish`) summed by the search wave of the NEXT launch -- none of which the
`sc_predict_batch` entry point runs.  Here the ORACLE's search (oracle/mcts.c, the restatement of src/mcts.rs:132-289) is
driven by an evaluator that calls the engine's public `predict` (L-predict of the C ABI: planes and action indices from
the oracle's own encoder, batch of one, `k_tower32` + `k_value_fc1` + `k_value_finish`), and the tree it builds must equal
the self-play handle's tree bit for bit: visit counts, value sums, uct words, priors, moves, paths.  A wrong meta column,
a different partial-sum order, a stale feature row or a plane that differs between the two encoders changes a value or a
prior in the last bit and shows up here.

Second half: the same comparison in distribution against the fp32 oracle network (what the reference's libtorch backend
computes, py/module.py:135-154), where bf16 / fp8 operand rounding makes the trees diverge chaotically."""
import numpy as np
import pytest

from helpers import GpuPredictEvaluator, _assert_same, random_games
from lines import LINES, SLOTS
from support import scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu


CASES = [(10, 128, "bf16"), (10, 256, "bf16"), (10, 128, "fp8"), (3, 256, "fp8")]
IDS = [f"{nb}x{C}_{p}" for nb, C, p in CASES]


@pytest.mark.parametrize("form", ["one_launch", "separate_launches"])
@pytest.mark.parametrize("nb,C,precision", CASES, ids=IDS)
def test_net_in_the_loop_lockstep_exact(scamd, orc, nb, C, precision, form):
    """180 simulations (BASELINE configs[1]'s rollout) from five positions inside a 64-slot handle (the other 59 slots play
    from the start position beside them): the slot's node pool equals the oracle search's that was fed the engine's own
    `predict` outputs -- after every simulation at first, then after bursts of 2-7 simulations (a host read completes the
    pending expansion in a launch of its own; inside a burst the expansion and its value tail run at the top of the next
    step launch, which is what production does)."""
    R = 180
    eng = scamd.Engine(nb, C, seed=21, precision=precision)
    sp = scamd.SelfPlay(eng, n_slots=64, n_games=64, rollout_num=R + 20, num_steps=4, cpuct=2.5, with_noise=False, seed=5)
    assert sp.launches_per_step() == 1      # whole 64-slot block: the one-launch step, value_head.ffn.0 tiles inside it
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
    done, burst = 0, [1] * 24 + [2, 3, 5, 7] * 40
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
            assert list(sp.slot(slot)["path"]) == list(srch.last_path()), (slot, done)
    assert done == R and sp.stats()["error_flags"] == 0
    for srch in searches:
        assert srch.dump()["n"][0] == R
    if form == "separate_launches":
        assert sp.timing(reset=False)["tower_launches"] >= R
    sp.close()
    eng.close()


@pytest.mark.parametrize("nb,C,precision", CASES, ids=IDS)
def test_net_in_the_loop_games_exact(scamd, orc, nb, C, precision):
    """whole self-play games with the network (ply transitions, temperature sampling in the first plies, tree reset, the
    history planes of a growing game line) in the production form -- nothing read between the launches -- equal the
    oracle's games played with the engine's `predict` as its evaluator: moves, root sums, children (N, Q, uct)."""
    cfg = dict(rollout_num=40, num_steps=7, cpuct=2.5, temperature=0.0, temperature_switch=3, with_noise=False)
    eng = scamd.Engine(nb, C, seed=22, precision=precision)
    sp = scamd.SelfPlay(eng, n_slots=64, n_games=64, seed=9, first_game_id=500, outcome_gate=100, **cfg)
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


def test_first_backup_is_predict_of_the_root(scamd, orc):
    """ADVICE r02's minimum: root priors and the first backed-up value of a self-play search equal `predict` on the root,
    here through the interactive handle (one slot: the two-launch form, k_step + k_value_fc1)."""
    eng = scamd.Engine(10, 128, seed=3)
    hip = scamd.ChessHip(eng)
    for line in LINES:
        steps, pri, val = hip.predict(line)
        sp = scamd.SelfPlay(eng, n_slots=1, n_games=1, rollout_num=50, num_steps=2, with_noise=False)
        sp.set_position(0, line)
        sp.enqueue(1)
        t = sp.tree(0)
        assert list(t["move"][1:]) == list(steps)
        assert np.array_equal(t["prior"][1:].view(np.uint32), np.asarray(pri, np.float32).view(np.uint32))
        assert t["n"][0] == 1 and np.float32(t["q"][0]).view(np.uint32) == np.float32(val).view(np.uint32)
        sp.close()
    eng.close()


# ---------------------------------------------------------------------------------- statistical, against the fp32 network
_ORACLE_ROOTS = {}   # (line) -> (moves, visit counts) of the fp32 oracle search: shared by the two precisions


def _oracle_root(orc, net, ln, R):
    key = " ".join(ln)
    if key not in _ORACLE_ROOTS:
        st = orc.State()
        for m in ln:
            st.push(m)
        srch = orc.Search(st)
        for _ in range(R):
            srch.sim(evaluator="orc_eval_net", user=net.h, cpuct=2.5, with_noise=False)
        d = srch.dump()
        fc, nc = int(d["first_child"][0]), int(d["n_child"][0])
        _ORACLE_ROOTS[key] = ([int(m) for m in d["move"][fc:fc + nc]], d["n"][fc:fc + nc].astype(np.float64))
    return _ORACLE_ROOTS[key]


@pytest.mark.parametrize("precision,tvd_bound,agree_bound", [("bf16", 0.01, 0.95), ("fp8", 0.06, 0.90)])
def test_search_statistics_against_the_fp32_oracle_network(scamd, orc, precision, tvd_bound, agree_bound):
    """The oracle's search with the oracle's fp32 network (py/module.py:135-154 restated, pinned by the reference module's
    vectors) against the engine's search with the bf16 / fp8 tower on 48 fixture positions at rollout 96: same weights,
    same search, only the network arithmetic differs.  A 1-ulp prior change can flip a near-tie and the trees then diverge
    (SURVEY.md 7), so the comparison is in distribution: mean total-variation distance of the root visit counts and the
    share of positions where the oracle's most visited move is (one of) the engine's most visited.  Bounds = about twice
    the values observed when the test was written (bf16: mean TVD 0.0029, max 0.021, 48/48; fp8: 0.0305, 0.063, 46/48); they
    are the build's own, the reference states none."""
    lines = [[orc.uci(m) for m in g[0]] for g in random_games(orc, 70, 60, seed=31) if g[1].legal_moves() and g[1].outcome() is None][:48]
    assert len(lines) == 48
    nb, Cw, R = 6, 128, 96
    eng = scamd.Engine(nb, Cw, seed=5, precision=precision)
    net = orc.Net(nb, Cw, seed=5)
    tv, agree = [], 0
    for ln in lines:
        omoves, on = _oracle_root(orc, net, ln, R)
        ge = scamd.search(eng, ln, R, cpuct=2.5)[1]
        assert [scamd.uci_move(c[0]) for c in ge] == omoves
        gn = np.asarray([c[1] for c in ge], np.float64)
        assert on.sum() == R - 1 and gn.sum() == R - 1
        tv.append(0.5 * np.abs(on / on.sum() - gn / gn.sum()).sum())
        agree += gn[int(np.argmax(on))] == gn.max()
    print(f"{precision} engine vs fp32 oracle, 48 positions, rollout {R}: mean root visit TVD {np.mean(tv):.4f} (max {np.max(tv):.4f}), "
          f"arg-max-visit agreement {agree}/48")
    assert np.mean(tv) < tvd_bound and agree / 48 >= agree_bound
    eng.close()
