"""GPU (-m gpu): search trees deeper than one 64-lane wavefront, from the locked positions of tests/deep_lines.py (whose depth
tests/test_deep_lines.py asserts on the oracle alone).

Every per-level structure of the device search is one entry per lane, so level 64 and beyond take a second code path that no
search from a position with many replies reaches: dev_expand backs up the first 64 path nodes from a prefetched register and the
rest in a `d = lane + 64` loop that re-reads path[] (the prefetch is unguarded: after a long path it holds stale entries that only
the `lane < plen` mask keeps out); `s_ps[depth]` / `path[depth]` past 20; the helper wave's DevChain reads of `s_ps` in the fused
step kernel; nodes with one child (no PUCT block: best_i stays 0, U is not written); and the depth limit of 1024 path nodes, which
the reference does not have.  Everything but the depth limit is compared with the CPU oracle bit for bit -- N, value sums, uct
words, child counts, moves, the length of the tree, the last path -- the depth limit against the closed form of a forced chain.

Not reached (out of scope): a repetition scan longer than 64 entries inside the TREE part of the chain -- it needs more than 64
forced, reversible, non-repeating plies and no such position is known; here positions repeat with period 4, so every leaf below
depth 8 carries both repetition flags (good for the planes the network sees) and its scan stops in the first round of lanes."""
import numpy as np
import pytest

import deep_lines as dl
from helpers import GpuPredictEvaluator, _assert_same, assert_same_tree_bits
from support import scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu

ERR_DEPTH_OVERFLOW = 8


def _assert_chain(t, s, where):
    """a forced line after s simulations, independently of the oracle: node i has the one child i + 1 and n[i] = s - i"""
    assert len(t["n"]) == s + 1, (where, len(t["n"]))
    assert np.array_equal(t["first_child"][:s], 1 + np.arange(s)), where
    assert np.array_equal(t["n_child"][:s], np.ones(s, np.int32)) and t["n_child"][s] == 0 and t["first_child"][s] == -1, where
    assert np.array_equal(t["n"], s - np.arange(s + 1)), (where, np.flatnonzero(t["n"] != s - np.arange(s + 1))[:8])


def _checked(s, R):
    """every simulation around the lane-round boundaries of the path (64, 128, 192), every 13th otherwise, the last four"""
    return 60 <= s <= 70 or 124 <= s <= 134 or 188 <= s <= 198 or s % 13 == 0 or s > R - 4


# ---------------------------------------------------------------------------------- synthetic evaluators: k_mcts
@pytest.mark.parametrize("evaluator", list(dl.EVALUATORS))
@pytest.mark.parametrize("name", list(dl.POSITIONS))
def test_deep_paths_lockstep_exact(scamd, orc, name, evaluator):
    """400 simulations from each position: the slot's node pool and last path equal the oracle's after the simulations around
    every 64-level boundary (and every 13th, and the last four).  FORCED: path s has s nodes, so simulations 65, 129 and 193 are
    the first to enter a new round of the backup loop; COMB: long and short paths alternate (stale path[] tails); SINK: the cached
    terminal at depth 1."""
    R = 400
    fen = dl.POSITIONS[name]
    sp = scamd.SelfPlay(None, n_slots=2, n_games=2, rollout_num=R + 1, num_steps=20, cpuct=2.5, with_noise=False, evaluator=evaluator, seed=3)
    sp.set_position(0, [], fen=fen)
    srch = orc.Search(orc.State(fen))
    longest = 0
    for s in range(1, R + 1):
        sp.enqueue(1)
        srch.sim(evaluator=dl.EVALUATORS[evaluator], cpuct=2.5, with_noise=False)
        if _checked(s, R):
            t, path = sp.tree(0), list(sp.slot(0)["path"])
            longest = max(longest, len(path))
            assert path == list(srch.last_path()), (s, len(path), len(srch.last_path()))
            assert_same_tree_bits(t, srch.dump(), s)
            if name in dl.FORCED:
                assert path == list(range(s)), s
                _assert_chain(t, s, s)
    print(f"{name} {evaluator}: longest compared path on the device {longest} nodes, tree of {len(sp.tree(0)['n'])} nodes")
    assert sp.tree(0)["n"][0] == R and sp.stats()["error_flags"] == 0
    assert longest == R if name in dl.FORCED else longest == 2 if name == "sink" else longest > 128
    sp.close()


# ---------------------------------------------------------------------------------- network in the loop: k_step, three launches
SLOTS = dict(zip((0, 17, 31, 40, 63), ("forced_w", "forced_b", "comb_w", "comb_b", "sink")))


@pytest.mark.parametrize("form", ["one_launch", "separate_launches"])
@pytest.mark.parametrize("nb,C,precision", [(10, 128, "bf16"), (3, 256, "fp8")], ids=["10x128_bf16", "3x256_fp8"])
def test_net_in_the_loop_deep_paths_exact(scamd, orc, nb, C, precision, form):
    """200 simulations from the five positions inside a 64-slot handle (the other 59 slots play from the start position): the
    slot's node pool equals the oracle search's that was fed the engine's own `predict` -- after every simulation up to 70 (levels
    64 to 70 each checked singly), then after bursts of 2-7.  In the one-launch form the helper wave reads `s_ps` through DevChain
    for the leaf's repetition flags (mailbox state 3) and for stage_history at depth 64 and beyond."""
    R = 200
    eng = scamd.Engine(nb, C, seed=21, precision=precision)
    sp = scamd.SelfPlay(eng, n_slots=64, n_games=64, rollout_num=R + 20, num_steps=4, cpuct=2.5, with_noise=False, seed=5)
    assert sp.launches_per_step() == 1
    if form == "separate_launches":
        sp.enable_timing(1)                 # every step timed: k_mcts, k_tower32 and k_value_fc1 as three launches
    searches, evs = {}, {}
    for slot, name in SLOTS.items():
        sp.set_position(slot, [], fen=dl.POSITIONS[name])
        searches[slot] = orc.Search(orc.State(dl.POSITIONS[name]))
        evs[slot] = GpuPredictEvaluator(orc, eng)
    done, longest = 0, dict.fromkeys(SLOTS, 0)
    for b in [1] * 70 + [2, 3, 5, 7] * 40:
        b = min(b, R - done)
        if b == 0:
            break
        sp.enqueue(b)
        sp.sync()
        done += b
        for slot, name in SLOTS.items():
            srch, ev = searches[slot], evs[slot]
            for _ in range(b):
                srch.sim(evaluator=ev.fn, cpuct=2.5, with_noise=False)
            t, path = sp.tree(slot), list(sp.slot(slot)["path"])
            _assert_same(t, srch.dump(), ev, (name, done))
            assert path == list(srch.last_path()), (name, done)
            longest[slot] = max(longest[slot], len(path))
            if name in dl.FORCED:
                assert path == list(range(done)), (name, done)
                _assert_chain(t, done, (name, done))
    print(f"{nb}x{C} {precision} {form}: longest path on the device " + ", ".join(f"{SLOTS[s]} {n}" for s, n in longest.items()))
    assert done == R and sp.stats()["error_flags"] == 0
    assert longest[0] == R and longest[17] == R and longest[63] == 2
    for slot in (31, 40):
        assert longest[slot] > 64, (SLOTS[slot], longest[slot])     # the network's comb: still past one wavefront
    if form == "separate_launches":
        assert sp.timing(reset=False)["tower_launches"] >= R
    sp.close()
    eng.close()


# ---------------------------------------------------------------------------------- ply transitions: a whole forced game
@pytest.mark.parametrize("name,plies", [("forced_w", 7), ("comb_b", 8)])
def test_forced_game_ply_by_ply(scamd, orc, name, plies):
    """a self-play game of 130 simulations a ply (every search ends more than 64 levels deep: the end-of-ply code follows a backup
    through both forms, and the next ply's root is a node the last search reached at depth 1): at every ply the root's children
    (move, N, Q) equal a fresh 130-simulation oracle search of that position, the move played is the first most-visited child, and
    the outcome is the oracle state's.  The game is the claimed threefold draw: the base returns at plies 4 and 8, and the claim
    already holds one ply earlier, when the only legal move repeats it for the third time (python-chess's
    can_claim_threefold_repetition) -- after 7 plies from FORCED, after 8 from COMB, whose first ply is the pawn move."""
    R = 130
    fen = dl.POSITIONS[name]
    sp = scamd.SelfPlay(None, n_slots=1, n_games=1, evaluator="synth", rollout_num=R, num_steps=12, outcome_gate=-1, temperature=0.0,
                        temperature_switch=0, with_noise=False, cpuct=2.5, seed=3)
    sp.set_position(0, [], fen=fen)
    sp.run()
    st = sp.stats()
    assert st["error_flags"] == 0 and st["games_finished"] == 1 and st["games_active"] == 0, st
    tr = sp.trace(0)
    state = orc.State(fen)
    for i, (mv, root_q, kids) in enumerate(tr["steps"]):
        srch, deepest = orc.Search(state), 0
        for _ in range(R):
            srch.sim(cpuct=2.5, with_noise=False)
            deepest = max(deepest, len(srch.last_path()))
        d = srch.dump()
        nc = int(d["n_child"][0])
        assert deepest > 64, (i, deepest)
        assert [(m, n, q) for m, n, q, _u in kids] == [(orc.uci(d["move"][1 + k]), int(d["n"][1 + k]), float(d["q"][1 + k])) for k in range(nc)], i
        assert np.float32(root_q).tobytes() == np.float32(d["q"][0]).tobytes() and sum(c[1] for c in kids) == R - 1, i
        assert mv == kids[int(np.argmax([c[1] for c in kids]))][0], i
        state.push(mv)
    assert tr["outcome"] == state.outcome() == {"termination": "ThreefoldRepetition", "winner": None}
    assert len(tr["steps"]) == plies
    sp.close()


# ---------------------------------------------------------------------------------- the depth limit
LAST_GOOD = 1024


def test_depth_limit_is_1024_path_nodes_and_callers_see_it(scamd, fen_mod):
    """dev_select (search_select.hpp) counts `depth` up once per level and raises ERR_DEPTH_OVERFLOW (8) when it reaches
    dmax = min(max_depth, DEPTH_LDS) = min(rollout + 2, 1024): depths 0 .. 1023 are walked, a path holds at most 1024 nodes.  On
    FORCED simulation s ends at depth s - 1, so simulation 1024 (a path of 1024 nodes, then a chain of 1025) is the last that raises
    no flag and simulation 1025 the first that does -- for every handle of rollout_num >= 1022, `Play`'s (60000) included.  The
    reference has no such limit and the oracle's path[ORC_MAX_PLY] is unchecked, so no oracle here: the closed form of the chain.
    On the flagged path every index stays in bounds (read off the code): the descent stops at depth 1023, so path[] and s_ps[] are
    written below dmax <= max_depth, DEPTH_LDS; the leaf's record goes to tpos[n_exp] with n_exp + 1 < tpos_cap kept by dev_expand,
    which also refuses children past node_cap.  A flagged tree is not the search's (the leaf below the limit is expanded again at
    every simulation), so no caller may hand out its numbers: sc_search returns -4, Play.mcts and fen.analyse raise."""
    pl = scamd.Play(None, fen=dl.FORCED_W, evaluator="synth")
    pl.mcts(LAST_GOOD - 1)
    pl.mcts(1)
    assert pl.sp.stats()["error_flags"] == 0
    assert list(pl.sp.slot(0)["path"]) == list(range(LAST_GOOD))
    _assert_chain(pl.sp.tree(0), LAST_GOOD, "last good")
    assert [(c[0], c[1]) for c in pl.inspect()[3]] == [("h1g1", LAST_GOOD - 1)]
    with pytest.raises(scamd.EngineError, match="error flags") as e:
        pl.mcts(1)
    assert e.value.code == -4 and e.value.flags & ERR_DEPTH_OVERFLOW
    assert pl.sp.stats()["error_flags"] & ERR_DEPTH_OVERFLOW
    pl.close()
    # analyse: the same boundary on a handle of its own
    got = fen_mod.analyse(None, [dl.FORCED_B], LAST_GOOD, evaluator="synth")["results"][0]
    assert [(c[0], c[1]) for c in got["children"]] == [("a8b8", LAST_GOOD - 1)]
    with pytest.raises(scamd.EngineError, match="error flags"):
        fen_mod.analyse(None, [dl.SINK, dl.FORCED_B], LAST_GOOD + 1, evaluator="synth")
    # sc_search_from, with the network
    eng = scamd.Engine(1, 128, seed=2)
    root_q, kids = scamd.search(eng, [], LAST_GOOD, fen=dl.FORCED_W)
    assert [(c[0], c[1]) for c in kids] == [("h1g1", LAST_GOOD - 1)]
    with pytest.raises(scamd.EngineError) as e:
        scamd.search(eng, [], 1100, fen=dl.FORCED_W)
    assert e.value.code == -4
    root_q, kids = scamd.search(eng, [], 30, fen=dl.FORCED_W)       # the next call starts clean
    assert [(c[0], c[1]) for c in kids] == [("h1g1", 29)]
    eng.close()


@pytest.fixture(scope="module")
def fen_mod(scamd):
    import scamd.fen as m
    return m
