"""GPU (-m gpu): sc_selfplay_report against tests/report_ref.py, bit for bit, applied to two sources: the device's own
SelfPlay.tree() of the same slot, and the oracle's tree after the same simulations (aligned as helpers.assert_same_tree_bits aligns
them).  The output arrays are pre-filled with support.FILL: what the call does not own keeps the pattern -- rows from n_lines on,
moves behind min(len, pv_cap), everything of a refused call."""
import json
import os

import numpy as np
import pytest

import deep_lines as dl
import lines
import report_ref as rr
from helpers import assert_same_tree_bits, san_to_move
from support import FILL, ROOT, run_torch_child, scamd_gpu, untouched  # noqa: F401

pytestmark = pytest.mark.gpu

ST_IDLE, ST_ACTIVE = 0, 1
LINE_KEYS = ("line_child", "line_n", "line_w", "line_prior", "line_len", "line_end")


def _report(scamd, sp, slots=None, multipv=1, pv_cap=64):
    from scamd import report as rp
    n = sp.cfg.n_slots if slots is None else len(slots)
    return rp.report(sp, slots, multipv, pv_cap, out=rp.report_arrays(n, multipv, pv_cap, fill=FILL))


def _check_entry(rep, i, t, turn, where, live=True, prior=True):
    """entry i of a report against report_ref on tree t"""
    multipv, cap = rep["pv"].shape[1:]
    ref = rr.report(t, turn, multipv, cap, live=live)
    for k in ("n_nodes", "n_root_children", "root_children_n", "root_n", "n_lines"):
        assert int(rep[k][i]) == ref[k], (where, k, int(rep[k][i]), ref[k])
    assert np.float32(rep["root_w"][i]).tobytes() == np.float32(ref["root_w"]).tobytes() and int(rep["turn"][i]) == turn, where
    nl = ref["n_lines"]
    got = rep.lines(i)
    assert len(got) == nl, where
    for r, x in enumerate(ref["lines"]):
        w = (where, "line", r)
        assert (int(rep["line_child"][i, r]), int(rep["line_n"][i, r]), int(rep["line_len"][i, r]), int(rep["line_end"][i, r])) == \
            (x["child"], x["n"], x["len"], x["end"]), w
        assert np.float32(rep["line_w"][i, r]).tobytes() == np.float32(x["w"]).tobytes(), w
        if prior:
            assert np.float32(rep["line_prior"][i, r]).tobytes() == np.float32(x["prior"]).tobytes(), w
        k = min(x["len"], cap)
        assert [int(m) for m in rep["pv"][i, r, :k]] == x["moves"] and untouched(rep["pv"][i, r, k:]), w
        g = got[r]
        assert (g["move"], g["pv"], g["n"], g["len"], g["end"], g["score"]) == (x["move"] if cap else None, x["pv"], x["n"], x["len"], x["end"], x["score"]), w
        assert np.float32(g["q"]).tobytes() == np.float32(x["q"]).tobytes(), w
    for k in LINE_KEYS:
        assert untouched(rep[k][i, nl:]), (where, k)
    assert untouched(rep["pv"][i, nl:]), where
    return ref


def _oracle(orc, st, sims, evaluator="synth", cpuct=2.5):
    srch = orc.Search(st)
    for _ in range(sims):
        srch.sim(evaluator=dl.EVALUATORS[evaluator], cpuct=cpuct, with_noise=False)
    return srch.dump()


def _handle(scamd, n_slots, evaluator="synth", rollout=512, **kw):
    return scamd.SelfPlay(None, **{**dict(n_slots=n_slots, n_games=n_slots, rollout_num=rollout, num_steps=20, cpuct=2.5, with_noise=False,
                                          evaluator=evaluator, seed=3, outcome_gate=1 << 30), **kw})


# ---------------------------------------------------------------------------------- the start position
@pytest.mark.parametrize("evaluator", ["synth", "synth_coarse", "synth_uniform"])
def test_start_position(scamd, orc, evaluator):
    """rollout 60 with each synthetic evaluator (synth_uniform: ties decide everything), multipv 1, 3 and 224"""
    sp = _handle(scamd, 1, evaluator)
    sp.enqueue(60)
    t, d = sp.tree(0), _oracle(orc, orc.State(), 60, evaluator)
    assert_same_tree_bits(t, d, evaluator)
    for multipv in (1, 3, 224):
        rep = _report(scamd, sp, None, multipv, 64)
        assert (int(rep["status"][0]), int(rep["ply"][0]), int(rep["sim"][0])) == (ST_ACTIVE, 0, 60)
        ref = _check_entry(rep, 0, t, rr.WHITE, (evaluator, multipv, "device tree"))
        _check_entry(rep, 0, d, rr.WHITE, (evaluator, multipv, "oracle"), prior=False)
        assert ref["n_lines"] == min(multipv, 20) and ref["root_children_n"] == 59
        assert rep.lines(0)[0]["move"] == scamd.move_uci(t["move"][1 + int(np.argmax(t["n"][1:21]))])
    assert sp.stats()["error_flags"] == 0
    sp.close()


# ---------------------------------------------------------------------------------- a root wider than a wavefront
@pytest.mark.parametrize("rollout", [40, 200])
def test_wide_root_all_ranks(scamd, orc, rollout):
    """lines.WIDE137: 137 root children, three rounds of 64 lanes; at 40 simulations most of them have no visit (ranked by index)"""
    sp = _handle(scamd, 2)
    sp.set_position(1, lines.WIDE137)
    sp.enqueue(rollout)
    t, d = sp.tree(1), _oracle(orc, lines.pushed(orc, lines.WIDE137), rollout)
    assert_same_tree_bits(t, d, rollout)
    for multipv in (137, 224, 100):
        rep = _report(scamd, sp, [1], multipv, 16)
        ref = _check_entry(rep, 0, t, rr.WHITE, (rollout, multipv, "device tree"))
        _check_entry(rep, 0, d, rr.WHITE, (rollout, multipv, "oracle"), prior=False)
        assert ref["n_lines"] == min(multipv, 137) and ref["n_root_children"] == 137
    sp.close()


# ---------------------------------------------------------------------------------- variations longer than a wavefront and than pv_cap
@pytest.mark.parametrize("evaluator", ["synth", "synth_uniform"])
def test_deep_variations(scamd, orc, evaluator):
    """the five locked positions at 200 simulations, pv_cap 64 and 1024: len is the walk's full length, min(len, pv_cap) moves are
    written.  forced: one line of 199 moves; comb: one-child nodes beside wide ones; sink: a cached terminal ends the line"""
    names = list(dl.POSITIONS)
    sp = _handle(scamd, len(names), evaluator)
    for i, name in enumerate(names):
        sp.set_position(i, [], fen=dl.POSITIONS[name])
    sp.enqueue(200)
    trees = [sp.tree(i) for i in range(len(names))]
    oracle = [_oracle(orc, orc.State(dl.POSITIONS[name]), 200, evaluator) for name in names]
    for i, name in enumerate(names):
        assert_same_tree_bits(trees[i], oracle[i], name)
    for cap in (64, 1024, 0):
        rep = _report(scamd, sp, None, 4, cap)
        for i, name in enumerate(names):
            turn = rr.WHITE if dl.POSITIONS[name].split()[1] == "w" else rr.BLACK
            d = oracle[i]
            ref = _check_entry(rep, i, trees[i], turn, (name, cap, "device tree"))
            _check_entry(rep, i, d, turn, (name, cap, "oracle"), prior=False)
            if name in dl.FORCED:
                assert [(x["len"], x["end"]) for x in ref["lines"]] == [(199, rr.END_OPEN)], name
            if name == "sink":
                assert [(x["len"], x["end"], x["score"]) for x in ref["lines"]] == [(1, rr.END_DRAW, ("cp", 0))]
            if name in dl.COMB:
                assert max(x["len"] for x in ref["lines"]) > 64 and ref["n_lines"] == 2, name
    assert sp.stats()["error_flags"] == 0
    sp.close()


# ---------------------------------------------------------------------------------- mate
def test_mate_scores(scamd, orc):
    """lines.MATED without its last move: the mating child, once expanded, is a decided terminal -> mate 1; one ply earlier the line
    g2g4 d8h4 is a mate against the side to move"""
    sp = _handle(scamd, 2, "synth_uniform")
    sp.set_position(0, lines.MATED[:3])
    sp.set_position(1, lines.MATED[:2])
    sp.enqueue(400)
    rep = _report(scamd, sp, None, 224, 8)
    for i, (cut, turn) in enumerate(((3, rr.BLACK), (2, rr.WHITE))):
        t = sp.tree(i)
        _check_entry(rep, i, t, turn, ("mate", cut))
        _check_entry(rep, i, _oracle(orc, lines.pushed(orc, lines.MATED[:cut]), 400, "synth_uniform"), turn, ("mate", cut, "oracle"), prior=False)
    top = rep.lines(0)[0]
    assert (top["pv"], top["end"], top["score"]) == (["d8h4"], rr.END_BLACK_WON, ("mate", 1)) and top["q"] == 1.0
    mated = [x for x in rep.lines(1) if x["pv"][:1] == ["g2g4"]]
    assert [(x["pv"], x["end"], x["score"]) for x in mated] == [(["g2g4", "d8h4"], rr.END_BLACK_WON, ("mate", -1))] and mated[0]["q"] < 0
    sp.close()


# ---------------------------------------------------------------------------------- empty reports
def test_empty_reports(scamd):
    """a root with no legal move, a fresh slot, an idle slot, a slot whose game has finished: n_lines == 0, the record is filled, the
    line rows keep the fill"""
    sp = scamd.SelfPlay(None, n_slots=4, n_games=3, rollout_num=8, num_steps=1, evaluator="synth", with_noise=False, seed=5, outcome_gate=1 << 30)
    sp.set_position(0, lines.MATED)          # White is mated: the game ends with its first search
    sp.set_position(1, ["e2e4"])             # fresh: no simulation yet
    rep = _report(scamd, sp, None, 3, 8)
    assert [int(x) for x in rep["n_lines"]] == [0, 0, 0, 0] and all(untouched(rep[k]) for k in LINE_KEYS + ("pv",))
    assert [int(x) for x in rep["status"]] == [ST_ACTIVE, ST_ACTIVE, ST_ACTIVE, ST_IDLE]
    assert [int(x) for x in rep["sim"][:3]] == [0, 0, 0] and [int(x) for x in rep["n_nodes"][:3]] == [1, 1, 1]
    assert [int(x) for x in rep["turn"]] == [rr.WHITE, rr.BLACK, rr.WHITE, -1] and [int(x) for x in rep["ply"][:2]] == [4, 1]
    sp.enqueue(3)                            # mid-ply: the root of slot 0 is a terminal (no legal move), 1 and 2 search
    rep = _report(scamd, sp, None, 3, 8)
    for i in range(4):
        s = sp.slot(i)
        assert (int(rep["status"][i]), int(rep["ply"][i]), int(rep["sim"][i])) == (s["status"], s["ply"], s["sim"]), i
    assert [int(x) for x in rep["n_lines"]] == [0, 3, 3, 0] and [int(x) for x in rep["sim"][:3]] == [3, 3, 3]
    _check_entry(rep, 0, sp.tree(0), rr.WHITE, "mated root")
    assert int(rep["root_n"][0]) == 3 and int(rep["n_root_children"][0]) == 0 and float(rep["root_w"][0]) == -3.0
    for _ in range(4):                       # num_steps = 1: every game ends with its first ply, nothing follows
        sp.enqueue(8)
    assert sp.stats()["games_active"] == 0
    rep = _report(scamd, sp, None, 3, 8)
    assert [int(x) for x in rep["n_lines"]] == [0, 0, 0, 0] and all(untouched(rep[k]) for k in LINE_KEYS + ("pv",))
    assert all(int(x) != ST_ACTIVE for x in rep["status"])
    for i in range(4):
        _check_entry(rep, i, sp.tree(i), int(rep["turn"][i]), ("finished", i), live=False)
    sp.close()


# ---------------------------------------------------------------------------------- slot subsets
def test_slot_subsets_and_refusals(scamd, orc):
    """five slots with different positions and simulation counts (some re-set after a search): subsets, orders, slots=None, n == 0;
    a duplicate or out-of-range slot is refused with nothing written"""
    from scamd import report as rp
    pos = [[], lines.WIDE, lines.WIDE137, lines.WIDE[:7], lines.MATED[:3]]
    sp = _handle(scamd, 5)
    for i, m in enumerate(pos):
        sp.set_position(i, m)
    sp.enqueue(30)
    sp.set_position(1, lines.WIDE[:4])       # a new search in slots 1 and 3: 17 simulations against 47
    sp.set_position(3, lines.WIDE)
    pos[1], pos[3] = lines.WIDE[:4], lines.WIDE
    sp.enqueue(17)
    sims = [47, 17, 47, 17, 47]
    trees = [sp.tree(i) for i in range(5)]
    turns = [rr.WHITE if len(m) % 2 == 0 else rr.BLACK for m in pos]
    for i in range(5):
        assert_same_tree_bits(trees[i], _oracle(orc, lines.pushed(orc, pos[i]), sims[i]), i)
    for slots in (None, [0], [4, 2], [3, 1, 0, 2, 4], [2, 3]):
        rep = _report(scamd, sp, slots, 5, 12)
        listed = list(range(5)) if slots is None else slots
        assert [int(s) for s in rep["slots"]] == listed
        for e, s in enumerate(listed):
            assert int(rep["sim"][e]) == sims[s] and int(rep["ply"][e]) == len(pos[s])
            _check_entry(rep, e, trees[s], turns[s], (slots, s))
    for bad in ([1, 1], [0, 5], [-1], [0, 1, 2, 3, 4, 0]):
        out = rp.report_arrays(len(bad), 5, 12, fill=FILL)
        with pytest.raises(scamd.EngineError) as e:
            rp.report(sp, bad, 5, 12, out=out)
        assert e.value.code == -1 and all(untouched(a) for a in out.values()), bad
    for multipv, cap in ((0, 4), (225, 4), (1, -1), (1, 1025)):
        assert sp.L.sc_selfplay_report(sp.h, 1, None, multipv, cap, *[None] * 8) == -1
    assert sp.L.sc_selfplay_report(sp.h, 6, None, 1, 4, *[None] * 8) == -1
    empty = _report(scamd, sp, [], 5, 12)
    assert len(empty["n_lines"]) == 0 and empty["pv"].shape == (0, 5, 12)
    assert sp.L.sc_selfplay_report(sp.h, 3, None, 2, 4, *[None] * 8) == 0       # every output may be NULL
    kernel_ms, total_ms = rp.last_timing(sp.L)
    assert 0 < kernel_ms < total_ms
    sp.close()


# ---------------------------------------------------------------------------------- no effect on play
def _play(scamd, make, reported):
    sp = make()
    n = 0
    while True:
        sp.enqueue(5)                        # not a divisor of the rollout of 12: reports fall mid-ply
        if reported:
            _report(scamd, sp, None, 7, 16)
            n += 1
        if sp.stats()["games_active"] == 0:
            break
    games = list(range(sp.cfg.n_games))
    out = sp.traces_json(games), sp.stats()
    sp.close()
    return out, n


@pytest.mark.parametrize("kind", ["selfplay", "match"])
def test_reports_do_not_change_the_games(scamd, kind):
    """two handles with the same seed, one reported on after every enqueue of 5 simulations: the traces of all games are the same
    bytes -- self-play with root noise, and a match handle with recycled slots"""
    if kind == "selfplay":
        make = lambda: scamd.SelfPlay(None, n_slots=4, n_games=4, rollout_num=12, num_steps=7, evaluator="synth", seed=9, outcome_gate=1 << 30)   # noqa: E731
    else:
        def make():
            sp = scamd.SelfPlay(None, n_slots=2, n_games=6, rollout_num=12, num_steps=9, evaluator="synth", seed=9, with_noise=False, outcome_gate=-1,
                                tie_random=True, cpuct=1.5)
            sp.set_match(None, None, 0x1111, 0x2222, colours=1)
            return sp
    (plain, st0), _ = _play(scamd, make, False)
    (seen, st1), n = _play(scamd, make, True)
    assert n > 10 and st0 == st1 and st0["error_flags"] == 0 and st0["games_finished"] == len(plain)
    assert seen == plain and all(len(t) > 200 for t in plain)


# ---------------------------------------------------------------------------------- analyse and san_lines
KIWI = "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1"


def test_analyse_keeps_its_keys_and_adds_lines(scamd, orc):
    from scamd import fen
    suite = [KIWI, dl.COMB_B, list(lines.PERFT)[2]]
    got = fen.analyse(None, suite, 40, cpuct=1.5, evaluator="synth", trees=True, multipv=3, pv_cap=12)["results"]
    for r, text in zip(got, suite):
        t = r["tree"]
        fc, nc = int(t["first_child"][0]), int(t["n_child"][0])
        # today's keys with today's values: the children from the tree, the move by numpy's argmax
        ch = [(scamd.move_uci(t["move"][fc + k]), int(t["n"][fc + k]), float(t["q"][fc + k]), float(t["prior"][fc + k])) for k in range(nc)]
        assert r["children"] == ch and r["move"] == ch[int(np.argmax([c[1] for c in ch]))][0] and r["fen"] == orc.State(text).fen()
        assert_same_tree_bits(t, _oracle(orc, orc.State(text), 40, cpuct=1.5), text)
        ref = rr.report(t, rr.WHITE if text.split()[1] == "w" else rr.BLACK, 3, 12)
        assert [(x["move"], x["pv"], x["n"], x["q"], x["len"], x["end"], x["score"]) for x in r["lines"]] == \
            [(x["move"], x["pv"], x["n"], x["q"], x["len"], x["end"], x["score"]) for x in ref["lines"]]
        assert len(r["lines"]) == min(3, nc) and r["pv"] == ref["lines"][0]["pv"] and r["score"] == ref["lines"][0]["score"]


_SAN_CHILD = """
import json, sys
import torch                      # first: libsc_engine.so then binds to the runtime torch loaded (moves_to_san works on torch's stream)
sys.path.insert(0, sys.argv[1])
import scamd
from scamd import report as rp
job = json.load(open(sys.argv[2]))
sp = scamd.SelfPlay(None, n_slots=2, n_games=2, rollout_num=512, num_steps=20, cpuct=2.5, with_noise=False, evaluator="synth", seed=3, outcome_gate=1 << 30)
sp.set_position(0, job["played"][0])
sp.set_position(1, job["played"][1], fen=job["fens"][1])
sp.enqueue(150)
rep = sp.report(multipv=4, pv_cap=10)
sans = rp.san_lines(rep, played=job["played"], fens=job["fens"])
print(json.dumps({"sans": sans, "pv": [[x["pv"] for x in rep.lines(i)] for i in range(2)], "len": [[x["len"] for x in rep.lines(i)] for i in range(2)]}))
"""


def test_san_lines(scamd, orc, tmp_path):
    """the variations of two middle-game positions (one from a FEN) as SAN: every SAN, replayed on the oracle through
    helpers.san_to_move, is the variation's move"""
    job = {"played": [lines.WIDE[:11], ["a2a4"]], "fens": [None, KIWI]}
    (tmp_path / "job.json").write_text(json.dumps(job))
    out = run_torch_child(tmp_path, _SAN_CHILD, os.path.join(ROOT, "smart-chess-rust_amd"), str(tmp_path / "job.json"), timeout=120)
    for i in range(2):
        pvs, sans = out["pv"][i], out["sans"][i]
        assert len(pvs) == len(sans) == 4 and max(out["len"][i]) > 2 and all(len(pv) == min(n, 10) for pv, n in zip(pvs, out["len"][i]))
        for pv, row in zip(pvs, sans):
            st = orc.State(job["fens"][i]) if job["fens"][i] else orc.State()
            for m in job["played"][i]:
                st.push(m)
            assert len(row) == len(pv)
            for san, m in zip(row, pv):
                assert orc.uci(san_to_move(st, san, orc)[0]) == m, (i, san, m)
                st.push(m)
