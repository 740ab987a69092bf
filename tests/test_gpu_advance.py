"""GPU (-m gpu): sc_selfplay_advance -- a move is played and the searched subtree below it is kept (csrc/advance_kernels.hip).

The yardstick is the CPU oracle, bit for bit and with no tolerance anywhere: after an advance into root child c the slot's
tree() is the oracle's dump of a FRESH search from the position after the move after N[c] simulations -- n, value sums, uct words,
moves, first_child, n_child -- because allocation order is expansion order (tests/test_advance_ref.py shows that on the oracle
alone), and a search that goes on from the kept tree stays equal to the oracle's that goes on from there.  Every test fails on a
library without the entry point."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import advance_ref as ar
import deep_lines as dl
import lines
from helpers import assert_same_tree_bits, random_games
from support import ROOT, scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu

ERR_POOL_OVERFLOW = 2
BIG_GATE = 1 << 30


def _handle(scamd, n_slots=1, rollout=2000, evaluator="synth", cpuct=2.5, gate=BIG_GATE, num_steps=200, **kw):
    return scamd.SelfPlay(None, n_slots=n_slots, n_games=kw.pop("n_games", n_slots), rollout_num=rollout, num_steps=num_steps, cpuct=cpuct,
                          with_noise=False, evaluator=evaluator, outcome_gate=gate, seed=3, **kw)


def _same(t, d, where):
    """a slot's tree() against an oracle dump: helpers.assert_same_tree_bits and first_child"""
    assert_same_tree_bits(t, d, where)
    assert ar.same_first_child(t, d), (where, "first_child")
    assert t["uct"].view(np.uint32)[0] == 0 and t["prior"].view(np.uint32)[0] == 0, (where, "root")


def _state(orc, moves=(), fen=None):
    st = orc.State(fen) if fen else orc.State()
    for m in moves:
        st.push(m)
    return st


def _children(d):
    """[(node, uci-less move, visits)] of a dump's root"""
    fc, nc = int(d["first_child"][0]), int(d["n_child"][0])
    return [(fc + k, int(d["move"][fc + k]), int(d["n"][fc + k])) for k in range(nc)]


def _most_visited(d):
    return max(_children(d), key=lambda c: (c[2], -c[0]))


def _snapshot(sp, slot):
    s = sp.slot(slot)
    fen = sp.fen(slot) if s["status"] == 1 else None   # (an idle slot holds no game)
    return sp.tree(slot), {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in s.items()}, fen


def _same_snapshot(a, b):
    return all(np.array_equal(a[0][k].view(np.uint8), b[0][k].view(np.uint8)) for k in a[0]) and a[1:] == b[1:]


# ---------------------------------------------------------------------------------- 1. re-root equals a fresh search
def test_reroot_equals_a_fresh_search(scamd, orc):
    """300 simulations from the start position on a handle built like Play's (rollout_num = 60000: a pool of 13 M nodes, of which
    the scratch must cover the live ones only), then the advance: into the most-visited child, the least-visited visited one and
    an unvisited one.  At 300 simulations every child of the start position has a visit (the oracle says so below), so the
    unvisited child is taken after 12 simulations, where most have none."""
    sp = _handle(scamd, rollout=60000, num_steps=4000)
    cases = 0
    for sims, pick in ((300, "most"), (300, "least"), (12, "unvisited")):
        sp.set_position(0, [])
        sp.enqueue(sims)
        d0 = ar.oracle_after(orc, orc.State(), sims).dump()
        kids = _children(d0)
        if sims == 300:
            assert min(c[2] for c in kids) >= 1 and len(d0["n"]) > 4 * 256
        c = {"most": _most_visited(d0), "least": min((k for k in kids if k[2] > 0), key=lambda k: (k[2], k[0])),
             "unvisited": next((k for k in kids if k[2] == 0), None)}[pick]
        assert c is not None and (c[2] == 0) == (pick == "unvisited")
        assert_same_tree_bits(sp.tree(0), d0, (pick, "before"))
        st, kept = sp.advance([0], [c[1]])
        fresh = ar.oracle_after(orc, _state(orc, [c[1]]), c[2])
        assert st == [0], (pick, st)
        _same(sp.tree(0), fresh.dump(), pick)
        assert kept.tolist() == [[len(fresh.dump()["n"]), 1 + fresh.num_evals(), c[2]]], (pick, kept)
        s = sp.slot(0)
        assert (s["ply"], s["sim"], s["status"], len(s["path"])) == (1, 0, 1, 0) and sp.fen(0) == _state(orc, [c[1]]).fen()
        assert sp.stats()["error_flags"] == 0
        cases += 1
    assert cases == 3
    sp.close()


# ---------------------------------------------------------------------------------- 2. the search continues on it
@pytest.mark.parametrize("evaluator,cpuct", [("synth", 2.5), ("synth_coarse", 2.5), ("synth", 1.5)])
def test_search_continues_on_the_kept_tree(scamd, orc, evaluator, cpuct):
    sp = _handle(scamd, evaluator=evaluator, cpuct=cpuct)
    sp.enqueue(300)
    d = ar.oracle_after(orc, orc.State(), 300, evaluator, cpuct).dump()
    played = []
    for step in range(2):   # the own move, then the reply
        c = _most_visited(d)
        played.append(c[1])
        st, kept = sp.advance([0], [c[1]])
        assert st == [0] and kept[0][2] == c[2]
        srch = ar.oracle_after(orc, _state(orc, played), c[2], evaluator, cpuct)
        _same(sp.tree(0), srch.dump(), (step, "advanced"))
        sp.enqueue(200)
        for _ in range(200):
            srch.sim(evaluator=dl.EVALUATORS[evaluator], cpuct=cpuct, with_noise=False)
        d = srch.dump()
        _same(sp.tree(0), d, (step, "200 more"))
        assert list(sp.slot(0)["path"]) == list(srch.last_path()) and int(d["n"][0]) == c[2] + 200
    assert sp.stats()["error_flags"] == 0
    sp.close()


# ---------------------------------------------------------------------------------- 3. shapes where the sweep can go wrong
SHAPES = {
    # name: (fen or None, moves from it, simulations, the move to advance with or None for the most-visited child)
    "forced_w": (dl.FORCED_W, [], 200, None),          # a chain of one-child nodes, 200 deep: one iteration of a chunk per node
    "forced_b": (dl.FORCED_B, [], 300, None),          # ... across a chunk boundary
    "comb_w": (dl.COMB_W, [], 260, None),
    "comb_b": (dl.COMB_B, [], 260, None),
    "wide137_below": (None, lines.WIDE137[:-1], 300, "f2g1b"),   # the kept root's block has 137 children
    "wide137_terminal": (None, lines.WIDE137, 300, None),        # the most-visited child ends the game: a terminal root
    "once": (None, [], 300, "once"),                   # a child visited exactly once: expanded, its children unvisited
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_where_the_sweep_can_go_wrong(scamd, orc, name):
    fen, moves, sims, pick = SHAPES[name]
    sp = _handle(scamd, rollout=1000)
    sp.set_position(0, moves, fen=fen)
    sp.enqueue(sims)
    base = _state(orc, moves, fen)
    d = ar.oracle_after(orc, base, sims).dump()
    assert_same_tree_bits(sp.tree(0), d, (name, "before"))
    kids = _children(d)
    if pick is None:
        c = _most_visited(d)
    elif pick == "once":
        c = next(k for k in kids if k[2] == 1)
    else:
        c = next(k for k in kids if orc.uci(k[1]) == pick)
    st, kept = sp.advance([0], [c[1]])
    after = base.copy()
    after.push(c[1])
    fresh = ar.oracle_after(orc, after, c[2]).dump()
    assert st == [0] and kept[0].tolist()[::2] == [len(fresh["n"]), c[2]], (name, st, kept)
    t = sp.tree(0)
    _same(t, fresh, name)
    if name.startswith("forced"):
        assert len(t["n"]) == sims and (t["n_child"][:-1] == 1).all() and np.array_equal(t["first_child"][:-1], 1 + np.arange(sims - 1))
    if name == "wide137_below":
        assert t["n_child"][0] == 137 and t["first_child"][0] == 1
    if name == "wide137_terminal":
        assert len(t["n"]) == 1 and t["first_child"][0] <= -2 and t["n"][0] == c[2] > 200
    if name == "once":
        assert t["n"][0] == 1 and len(t["n"]) == 1 + t["n_child"][0] and (t["n"][1:] == 0).all()
    # the search goes on from it
    sp.enqueue(50)
    srch = ar.oracle_after(orc, after, c[2] + 50)
    _same(sp.tree(0), srch.dump(), (name, "50 more"))
    assert sp.stats()["error_flags"] == 0
    sp.close()


@pytest.mark.parametrize("gate,want", [(-1, 1), (BIG_GATE, 0)])
def test_terminal_child_the_mate_in_one(scamd, orc, gate, want):
    """MATED's last move mates: with outcome_gate = -1 the advance ends the game (status 1, the trace's outcome), with a large
    gate the game goes on from a terminal root that holds the child's visits"""
    sp = _handle(scamd, rollout=1000, gate=gate)
    sp.set_position(0, lines.MATED[:3])
    sp.enqueue(100)
    d = ar.oracle_after(orc, _state(orc, lines.MATED[:3]), 100).dump()
    c = next(k for k in _children(d) if orc.uci(k[1]) == lines.MATED[3])
    assert c[2] > 1
    st, kept = sp.advance([0], [lines.MATED[3]])
    assert st == [want]
    if want == 1:
        tr = sp.trace(0)
        assert tr["outcome"] == {"termination": "Checkmate", "winner": "Black"} and [s[0] for s in tr["steps"]] == [lines.MATED[3]]
        assert [(k[0], k[1]) for k in tr["steps"][0][2]] == [(orc.uci(m), n) for _, m, n in _children(d)]
        assert kept.tolist() == [[0, 0, 0]] and sp.stats()["games_finished"] == 1
    else:
        t = sp.tree(0)
        _same(t, ar.oracle_after(orc, _state(orc, lines.MATED), c[2]).dump(), "terminal root")
        assert kept.tolist() == [[1, 1, c[2]]] and t["first_child"][0] <= -2
        sp.enqueue(5)
        assert sp.tree(0)["n"].tolist() == [c[2] + 5]
        assert sp.advance([0], ["e2e4"])[0] == [-1]   # no move is playable on a terminal root
    assert sp.stats()["error_flags"] == 0
    sp.close()


# ---------------------------------------------------------------------------------- 4. many slots, one call
def test_many_slots_one_call(scamd, orc):
    """64 slots with different lines and different moves in one call, next to 64 oracle searches; eight more slots, searched as
    far but not listed, keep every byte"""
    games = [g for g, st in random_games(orc, 140, 14, seed=21) if st.legal_moves() and not st.outcome()][:72]
    assert len(games) == 72
    sp = _handle(scamd, n_slots=72, rollout=400)
    for g, mv in enumerate(games):
        sp.set_position(g, mv)
    sp.enqueue(120)
    listed = [g for g in range(72) if g % 9 != 4]
    quiet = [g for g in range(72) if g % 9 == 4]
    before = {g: _snapshot(sp, g) for g in quiet}
    rep_before = sp.report(quiet, multipv=4)
    picks, fresh = [], []
    for g in listed:
        st0 = _state(orc, games[g])
        kids = _children(ar.oracle_after(orc, st0, 120).dump())
        c = kids[(5 * g + 1) % len(kids)]
        picks.append(c)
        st0.push(c[1])
        fresh.append(ar.oracle_after(orc, st0, c[2]))
    status, kept = sp.advance(listed, [c[1] for c in picks])
    assert status == [0] * 64
    assert len({c[2] for c in picks}) > 5 and any(c[2] == 0 for c in picks)
    for i, g in enumerate(listed):
        d = fresh[i].dump()
        _same(sp.tree(g), d, g)
        assert kept[i].tolist() == [len(d["n"]), 1 + fresh[i].num_evals(), picks[i][2]], g
        assert sp.slot(g)["ply"] == len(games[g]) + 1
    for g in quiet:
        assert _same_snapshot(before[g], _snapshot(sp, g)), g
    rep_after = sp.report(quiet, multipv=4)
    assert all(np.array_equal(np.asarray(rep_before[k]), np.asarray(rep_after[k])) for k in ("n_nodes", "sim", "ply", "line_n", "pv", "root_n"))
    # ... and all 72 search on, the listed ones from what was kept
    sp.enqueue(30)
    for i, g in enumerate(listed[:16]):
        for _ in range(30):
            fresh[i].sim(cpuct=2.5, with_noise=False)
        _same(sp.tree(g), fresh[i].dump(), (g, "30 more"))
    assert sp.stats()["error_flags"] == 0
    sp.close()


# ---------------------------------------------------------------------------------- 5. trace and line
def test_trace_step_is_the_searched_plys(scamd, orc):
    """a twin with rollout_num = 300 and temperature 0 ends its ply on the device; the advance with the twin's move after 300
    simulations writes the same trace step.  num_steps = 1 ends both games there, which makes the traces readable"""
    mv = ["e2e4", "c7c5"]
    twin = _handle(scamd, rollout=300, num_steps=1, temperature=0.0, temperature_switch=0)
    twin.set_position(0, mv)
    twin.enqueue(300)
    twin.sync()
    want = twin.trace(0)
    assert want is not None and len(want["steps"]) == 1
    sp = _handle(scamd, rollout=1000, num_steps=1, temperature=0.0, temperature_switch=0)
    sp.set_position(0, mv)
    sp.enqueue(300)
    assert sp.trace(0) is None
    st, kept = sp.advance([0], [want["steps"][0][0]])
    assert st == [1]                       # num_steps: the game ends with this ply, as the twin's did
    got = sp.trace(0)
    assert got["steps"] == want["steps"] and got["outcome"] == want["outcome"]
    assert sum(k[1] for k in got["steps"][0][2]) == 299
    # ... and a move that is NOT the most visited records the same distribution, with that move as the ply's
    sp2 = _handle(scamd, rollout=1000, num_steps=1)
    sp2.set_position(0, mv)
    sp2.enqueue(300)
    other = min(want["steps"][0][2], key=lambda k: k[1])[0]
    assert other != want["steps"][0][0] and sp2.advance([0], [other])[0] == [1]
    got2 = sp2.trace(0)
    assert got2["steps"][0][0] == other and got2["steps"][0][1:] == want["steps"][0][1:]
    for h in (twin, sp, sp2):
        assert h.stats()["error_flags"] == 0
        h.close()


def test_line_agrees_with_set_position(scamd, orc):
    """fen, ply and what the next simulations see (the synthetic evaluator hashes the position; repetition flags enter the
    outcome) agree with a handle set to the longer list; a knight shuffle makes the advanced position a repetition"""
    mv = ["g1f3", "g8f6", "f3g1", "f6g8", "g1f3", "g8f6", "f3g1"]
    a, b = _handle(scamd, rollout=1000), _handle(scamd, rollout=1000)
    a.set_position(0, mv)
    a.enqueue(100)
    t = a.tree(0)
    fc, nc = int(t["first_child"][0]), int(t["n_child"][0])
    k = next(i for i in range(nc) if scamd.move_uci(t["move"][fc + i]) == "f6g8")
    n_c = int(t["n"][fc + k])
    st, kept = a.advance([0], ["f6g8"])
    b.set_position(0, mv + ["f6g8"])
    assert st == [0] and a.fen(0) == b.fen(0) == _state(orc, mv + ["f6g8"]).fen() and a.slot(0)["ply"] == b.slot(0)["ply"] == 8
    b.enqueue(n_c)
    for h in (a, b):
        h.enqueue(60)
    ta, tb = a.tree(0), b.tree(0)
    for key in ("n", "q", "first_child", "n_child"):
        assert np.array_equal(ta[key].view(np.uint32), tb[key].view(np.uint32)), key
    for key in ("uct", "prior", "move"):
        assert np.array_equal(ta[key][1:].view(np.uint8), tb[key][1:].view(np.uint8)), key
    _same(ta, ar.oracle_after(orc, _state(orc, mv + ["f6g8"]), n_c + 60).dump(), "oracle")
    a.close()
    b.close()


def test_unexpanded_root_is_push_moves(scamd, orc):
    a, b = _handle(scamd, rollout=1000, num_steps=2), _handle(scamd, rollout=1000, num_steps=2)
    for h in (a, b):
        h.set_position(0, ["d2d4"])
    st, kept = a.advance([0], ["g8f6"])
    assert st == [0] and kept.tolist() == [[1, 1, 0]] and b.push_moves([0], ["g8f6"]) == [0]
    assert _same_snapshot(_snapshot(a, 0), _snapshot(b, 0))
    assert a.advance([0], ["e2e5"])[0] == [-1] and a.advance([0], ["c2c4"])[0] == [1] and b.push_moves([0], ["c2c4"]) == [1]
    ta, tb = a.trace(0), b.trace(0)
    assert ta == tb and [s[0] for s in ta["steps"]] == ["g8f6", "c2c4"] and sum(k[1] for k in ta["steps"][0][2]) == 1
    a.close()
    b.close()


# ---------------------------------------------------------------------------------- 6. refusals change nothing
def test_refusals_change_nothing(scamd, orc):
    sp = _handle(scamd, n_slots=3, n_games=2, rollout=1000)     # slot 2 draws no game: idle
    sp.enqueue(80)
    assert sp.slot(2)["status"] == 0
    before = [_snapshot(sp, g) for g in range(3)]
    # an illegal move, a move of the other side (legal elsewhere, no child here), an idle slot -- in one call
    st, kept = sp.advance([0, 1, 2], ["e2e5", "e7e5", "e2e4"])
    assert st == [-1, -1, -2] and kept.tolist() == [[0, 0, 0]] * 3
    assert sp.advance([], [])[0] == []
    for bad in ([0, 0], [0, 3], [-1]):
        with pytest.raises(scamd.EngineError, match="advance: slot"):
            sp.advance(bad, ["e2e4"] * len(bad))
    assert all(_same_snapshot(before[g], _snapshot(sp, g)) for g in range(3))
    # a refused entry next to an accepted one: the accepted one advances, the other keeps every byte
    d = ar.oracle_after(orc, orc.State(), 80).dump()
    c = _most_visited(d)
    st, kept = sp.advance([1, 0], ["a1a8", c[1]])
    assert st == [-1, 0] and kept[0].tolist() == [0, 0, 0] and kept[1][2] == c[2]
    assert _same_snapshot(before[1], _snapshot(sp, 1)) and _same_snapshot(before[2], _snapshot(sp, 2))
    _same(sp.tree(0), ar.oracle_after(orc, _state(orc, [c[1]]), c[2]).dump(), "accepted")
    assert sp.stats()["error_flags"] == 0
    sp.close()
    # handles the call is not for
    ext = scamd.SelfPlay(None, n_slots=2, n_games=2, rollout_num=8, num_steps=10, with_noise=False, evaluator="synth", outcome_gate=-1)
    ext.set_external(None, 0, 0)
    with pytest.raises(scamd.EngineError, match="external"):
        ext.advance([0], ["e2e4"])
    ext.close()
    rf = scamd.SelfPlay(None, n_slots=1, n_games=1, rollout_num=300, num_steps=10, with_noise=False, evaluator="synth", rollout_factor=2.0)
    rf.enqueue(5)
    snap = _snapshot(rf, 0)
    with pytest.raises(scamd.EngineError, match="rollout_factor"):
        rf.advance([0], ["e2e4"])
    assert _same_snapshot(snap, _snapshot(rf, 0))
    rf.close()


# ---------------------------------------------------------------------------------- 7. the pool holds only the live tree
def test_the_pool_holds_only_the_live_tree(scamd, orc):
    """rollout_num = 400 sizes the pool for 400 evaluations; 12 plies of up to 200 simulations each run far more than that in
    total, because every advance compacts the pool to the kept subtree"""
    R = 400
    sp = _handle(scamd, rollout=R)
    st, srch, n_exp, total = orc.State(), None, 1, 0
    srch = orc.Search(st)
    for ply in range(12):
        k = min(200, R - n_exp)
        assert k > 0
        sp.enqueue(k)
        total += k
        for _ in range(k):
            srch.sim(cpuct=2.5, with_noise=False)
        d = srch.dump()
        c = _most_visited(d)
        status, kept = sp.advance([0], [c[1]])
        assert status == [0], (ply, status)
        st.push(c[1])
        srch = ar.oracle_after(orc, st, c[2])
        _same(sp.tree(0), srch.dump(), ply)
        n_exp = int(kept[0][1])
        assert n_exp == 1 + srch.num_evals() and sp.stats()["error_flags"] & ERR_POOL_OVERFLOW == 0
    print(f"12 plies, {total} simulations on a pool for {R}")
    assert total > 3 * R and sp.stats()["error_flags"] == 0 and sp.slot(0)["ply"] == 12
    sp.close()


# ---------------------------------------------------------------------------------- 8. network in the loop, fused launch form
@pytest.mark.parametrize("precision", ["bf16", "fp8"])
def test_network_in_the_loop_fused(scamd, orc, precision):
    """64 slots on a 1 x 128 network in the one-launch form: 40 simulations, the advance of every slot into its most-visited
    child, 40 more -- against a second handle that searched the advanced positions fresh for N[c] + 40 simulations.  k_step
    prefetches the root's child block at nodes 1.. and reads the root's position from tpos[0]: both must hold on the compacted
    layout.  The fresh handle steps all slots together, so each slot's tree is read when the handle has run that slot's count."""
    games = [g for g, st in random_games(orc, 130, 10, seed=8) if st.legal_moves() and not st.outcome()][:64]
    eng = scamd.Engine(1, 128, seed=2, precision=precision)
    a = scamd.SelfPlay(eng, n_slots=64, n_games=64, rollout_num=200, num_steps=100, with_noise=False, seed=5, outcome_gate=BIG_GATE)
    b = scamd.SelfPlay(eng, n_slots=64, n_games=64, rollout_num=200, num_steps=100, with_noise=False, seed=5, outcome_gate=BIG_GATE)
    assert a.launches_per_step() == 1 and b.launches_per_step() == 1
    for g, mv in enumerate(games):
        a.set_position(g, mv)
    a.enqueue(40)
    a.sync()
    moves, counts = [], []
    for g in range(64):
        t = a.tree(g)
        fc, nc = int(t["first_child"][0]), int(t["n_child"][0])
        k = int(np.argmax(t["n"][fc:fc + nc]))
        moves.append(int(t["move"][fc + k]))
        counts.append(int(t["n"][fc + k]))
    status, kept = a.advance(list(range(64)), moves)
    assert status == [0] * 64 and kept[:, 2].tolist() == counts
    a.enqueue(40)
    a.sync()
    for g, mv in enumerate(games):
        b.set_position(g, list(mv) + [moves[g]])
    done, seen = 0, 0
    for target in sorted(set(counts)):
        b.enqueue(target + 40 - done)
        b.sync()
        done = target + 40
        for g in [g for g in range(64) if counts[g] == target]:
            ta, tb = a.tree(g), b.tree(g)
            assert len(ta["n"]) == len(tb["n"]), (g, len(ta["n"]), len(tb["n"]))
            for key in ("n", "q", "first_child", "n_child"):
                assert np.array_equal(ta[key].view(np.uint32), tb[key].view(np.uint32)), (g, key)
            for key in ("uct", "prior", "move"):
                assert np.array_equal(ta[key][1:].view(np.uint8), tb[key][1:].view(np.uint8)), (g, key)
            assert ta["n"][0] == target + 40
            seen += 1
    assert seen == 64 and a.stats()["error_flags"] == 0 and b.stats()["error_flags"] == 0
    a.close()
    b.close()
    eng.close()


# ---------------------------------------------------------------------------------- 9. Play(keep_tree=True) and the UCI tool
def test_play_keeps_its_tree(scamd, orc):
    pl = scamd.Play(None, evaluator="synth", keep_tree=True)
    pl.mcts(300)
    d = ar.oracle_after(orc, orc.State(), 300).dump()
    c = _most_visited(d)
    assert pl.step() == orc.uci(c[1])
    assert pl.inspect()[1] == [orc.uci(c[1])] and pl.sp.tree(0)["n"][0] == c[2]
    pl.mcts(200)
    t = pl.sp.tree(0)
    assert t["n"][0] == c[2] + 200 > 200
    _same(t, ar.oracle_after(orc, _state(orc, [c[1]]), c[2] + 200).dump(), "play")
    pl.apply_move("a2a1")                      # not playable: the fresh node of the default
    assert len(pl.sp.tree(0)["n"]) == 1 and pl.moves[-1] == "a2a1"
    pl.close()
    fresh = scamd.Play(None, evaluator="synth")
    fresh.mcts(300)
    fresh.step()
    assert len(fresh.sp.tree(0)["n"]) == 1     # the default stays as it was
    fresh.close()


TOOL = os.path.join(ROOT, "tools", "uci_engine.py")


def _wait(pr, prefix, timeout=30.0):
    """read to the first line that starts with `prefix` (which may hold blanks) and return it"""
    deadline = time.monotonic() + timeout
    while True:
        ln = pr.readline(deadline)
        if ln.startswith(prefix):
            return ln


def test_uci_tool_keeps_its_tree(scamd, orc):
    from scamd import external as ext
    pr = ext._UciProc([sys.executable, TOOL, "--evaluator", "synth", "--keep-tree"])
    try:
        pr.send("uci")
        deadline = time.monotonic() + 90
        opts = []
        while True:
            ln = pr.readline(deadline)
            if ln.startswith("option name"):
                opts.append(ln)
            if ln == "uciok":
                break
        assert "option name KeepTree type check default true" in opts
        pr.send("setoption name Chunk value 4096")
        pr.send("position startpos")
        pr.send("go nodes 200")
        best = pr.wait_for("bestmove", 30).split()[1]
        st = orc.State()
        assert best in st.legal_uci()
        st.push(best)
        reply = st.legal_uci()[0]
        st.push(reply)
        pr.send(f"position startpos moves {best} {reply}")
        pr.send("go nodes 200")
        words = _wait(pr, "info string kept").split()
        nodes, visits = int(words[3]), int(words[5])
        assert words[4] == "nodes" and words[6] == "visits" and nodes >= 1 and visits >= 0
        info = _wait(pr, "info depth").split()
        assert int(info[info.index("nodes") + 1]) == 200          # 200 MORE simulations
        best2 = pr.wait_for("bestmove", 30).split()[1]
        assert best2 in st.legal_uci()
        # a position that does not extend the game restarts: no kept line in front of the next answer
        pr.send("position startpos moves d2d4")
        pr.send("go nodes 50")
        deadline = time.monotonic() + 30
        while True:
            ln = pr.readline(deadline)
            assert not ln.startswith("info string kept")
            if ln.startswith("bestmove"):
                break
        pr.send("quit")
        assert pr.p.wait(timeout=30) == 0
    finally:
        if pr.p.poll() is None:
            pr.p.kill()
        pr.reap(time.monotonic() + 5)


# ---------------------------------------------------------------------------------- 10. the rate tool at tiny sizes
def test_advance_rate_prints_its_lines():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "advance_rate.py"), "--slots", "8", "--rollouts", "24", "--big", "300,600",
                        "--reps", "1", "--blocks", "1", "--channels", "128", "--game-nodes", "40", "--game-moves", "2", "--out", os.devnull],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    out = [json.loads(ln) for ln in r.stdout.splitlines()]
    print(r.stdout)
    kinds = [ln["kind"] for ln in out]
    assert kinds == ["call", "one_slot", "one_slot", "kept_share", "kept_share", "uci_game", "uci_game"]
    for ln in out:
        assert ln["tool"] == "advance_rate" and ln["error_flags"] == 0
    call = out[0]
    assert call["slots"] == 8 and call["rollout"] == 24 and call["same_position"] is True
    for k in ("advance_ms", "set_position_ms"):
        med, lo, hi = call[k]
        assert 0 < lo <= med <= hi
    for ln in out[1:3]:
        assert ln["nodes"] >= 300 and ln["advance_ms"][0] > 0 and ln["kept_nodes"] >= 1
    for ln, ev in zip(out[3:5], ("synth", "net")):
        assert ln["evaluator"] == ev and 0 < ln["share_own_move"] <= 1 and 0 <= ln["share_after_reply"] <= ln["share_own_move"]
    assert [ln["keep_tree"] for ln in out[5:]] == [False, True]
    assert out[5]["kept_visits"] == 0 and out[6]["kept_visits"] >= 0 and all(ln["nps"] > 0 and ln["moves"] == 2 for ln in out[5:])
