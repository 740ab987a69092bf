"""CPU: the two facts sc_selfplay_advance rests on, on the oracle alone, and the UCI protocol's KeepTree over a stub searcher.

(1) Indices only grow downward in the tree (a node's child block is allocated behind it), so one ascending sweep marks a
subtree; (2) the stable compaction of the subtree below root child c IS the tree of a fresh search from the position after c's
move after N[c] simulations -- allocation order is expansion order -- array for array: n, value sums, uct words, moves,
first_child, n_child.  tests/advance_ref.py's reroot is that sweep and compaction in numpy; tests/test_gpu_advance.py holds the
device to the same oracle."""
import queue

import numpy as np
import pytest

import advance_ref as ar
import deep_lines as dl
from helpers import assert_same_tree_bits

LINE3 = ["e2e4", "c7c5", "g1f3"]


@pytest.mark.parametrize("evaluator", list(dl.EVALUATORS))
@pytest.mark.parametrize("line", [[], LINE3], ids=["start", "line3"])
def test_reroot_of_every_root_child_is_the_fresh_search(orc, line, evaluator):
    st = orc.State()
    for m in line:
        st.push(m)
    d = ar.oracle_after(orc, st, 400, evaluator).dump()
    fc, nc = int(d["first_child"][0]), int(d["n_child"][0])
    assert fc == 1 and nc >= 20 and (d["first_child"][d["first_child"] >= 0] > np.flatnonzero(d["first_child"] >= 0)).all()
    visited = 0
    for c in range(fc, fc + nc):
        st2 = st.copy()
        st2.push(int(d["move"][c]))
        fresh = ar.oracle_after(orc, st2, int(d["n"][c]), evaluator).dump()
        got = ar.reroot(d, c)
        assert_same_tree_bits(got, fresh, (line, evaluator, c))
        assert ar.same_first_child(got, fresh) and np.array_equal(got["first_child"], fresh["first_child"]), c
        assert np.array_equal(got["parent"], fresh["parent"]), c
        visited += d["n"][c] > 0
    assert visited >= 5 and sum(int(d["n"][c]) for c in range(fc, fc + nc)) == 399


def test_reroot_on_a_forced_chain(orc):
    """one-child nodes: every block of the sweep is marked by the node right in front of it"""
    st = orc.State(dl.FORCED_W)
    d = ar.oracle_after(orc, st, 120).dump()
    assert len(d["n"]) == 121 and int(d["n_child"][0]) == 1
    st.push("h1g1")
    fresh = ar.oracle_after(orc, st, 119).dump()
    got = ar.reroot(d, 1)
    assert_same_tree_bits(got, fresh, "forced")
    assert np.array_equal(got["first_child"], fresh["first_child"])
    # ... and twice: the reply as well
    st.push("a8b8")
    assert_same_tree_bits(ar.reroot(got, 1), ar.oracle_after(orc, st, 118).dump(), "forced twice")


def test_reroot_keeps_nothing_outside_the_subtree():
    t = dict(n=np.array([5, 3, 1, 1, 1, 0], np.int32), q=np.zeros(6, np.float32), uct=np.ones(6, np.float32), move=np.arange(6, dtype=np.uint16),
             first_child=np.array([1, 3, 5, -1, -3, -1], np.int32), n_child=np.array([2, 2, 1, 0, 0, 0], np.int32))
    a, b = ar.reroot(t, 1), ar.reroot(t, 2)
    assert a["n"].tolist() == [3, 1, 1] and a["first_child"].tolist() == [1, -1, -3] and a["uct"].tolist() == [0, 1, 1]
    assert b["n"].tolist() == [1, 0] and b["first_child"].tolist() == [1, -1] and b["move"].tolist() == [2, 5]
    assert ar.reroot(t, 3)["n"].tolist() == [1]


# ------------------------------------------------------------------ the protocol's KeepTree over a stub searcher
def _serve(commands, stub):
    from scamd import uci
    out, q = [], queue.Queue()
    for c in commands:
        q.put(c)
    q.put(None)
    p = uci.Protocol(stub, out.append)
    p.opt["Chunk"] = 4096   # one chunk per search: one info line per `go`, the last
    assert p.run(q) == 0
    return out, p


GAME = ["position startpos moves e2e4", "go nodes 90", "position startpos moves e2e4 e7e5 g1f3", "go nodes 30"]


def test_keeptree_is_offered_and_off_by_default():
    s = ar.KeepStub()
    out, p = _serve(["uci"] + GAME, s)
    assert "option name KeepTree type check default false" in out and p.opt["KeepTree"] is False
    assert not [ln for ln in out if ln.startswith("info string kept")]
    # every position is set up, every search starts afresh
    assert [c[0] for c in s.log] == ["set_position", "set_position", "start", "set_position", "start", "close"]
    assert all(c[1] is False for c in s.log if c[0] == "start")
    assert [ln.split()[ln.split().index("nodes") + 1] for ln in out if ln.startswith("info depth")] == ["90", "30"]


def test_keeptree_advances_an_extending_position():
    s = ar.KeepStub()
    out, p = _serve(["setoption name KeepTree value true"] + GAME + ["go nodes 10"], s)
    assert p.opt["KeepTree"] is True
    # 90 visits, two advances keep a third each time: 30, then 10
    assert ("advance", "e7e5", 30) in s.log and ("advance", "g1f3", 10) in s.log
    assert [ln for ln in out if ln.startswith("info string kept")] == ["info string kept 71 nodes 10 visits"]
    assert [c for c in s.log if c[0] == "start"] == [("start", False), ("start", True), ("start", True)]
    assert [c[0] for c in s.log].count("set_position") == 2          # the constructor's and the first position's
    # go nodes N runs N MORE simulations: the searcher was asked for 30 and for 10 on the kept tree
    assert [ln.split()[ln.split().index("nodes") + 1] for ln in out if ln.startswith("info depth")] == ["90", "30", "10"]
    assert s.visits == 10 + 30 + 10
    assert [ln for ln in out if ln.startswith("bestmove")] == ["bestmove e2e4"] * 3


def test_keeptree_restarts_on_anything_else():
    # a position that does not extend the current one; another base; ucinewgame; a refused move
    for second, refuse in (("position startpos moves d2d4 d7d5", ()), ("position startpos", ()),
                           ("position fen " + dl.SINK + " moves h1g1", ()), ("position startpos moves e2e4", ()),
                           ("position startpos moves e2e4 e7e5 g1f3", ("g1f3",))):
        s = ar.KeepStub(refuse)
        out, p = _serve(["setoption name KeepTree value true", GAME[0], GAME[1], second, "go nodes 20"], s)
        assert not [ln for ln in out if ln.startswith("info string kept")], second
        assert [c for c in s.log if c[0] == "start"] == [("start", False), ("start", False)], second
        sets = [c for c in s.log if c[0] == "set_position"]
        assert len(sets) == 3 and sets[-1][2] == second.split("moves")[1].split() if "moves" in second else sets[-1][2] == [], second
        assert ("refused", "g1f3") in s.log if refuse else not [c for c in s.log if c[0] == "refused"]
    s = ar.KeepStub()
    out, p = _serve(["setoption name KeepTree value true", GAME[0], GAME[1], "ucinewgame", GAME[2], "go nodes 20"], s)
    assert not [ln for ln in out if ln.startswith("info string kept")] and not [c for c in s.log if c[0] == "advance"]
    assert [c for c in s.log if c[0] == "start"] == [("start", False), ("start", False)]
    # switching the option restarts as well, and a wrong value is named
    s = ar.KeepStub()
    out, p = _serve(["setoption name KeepTree value true", GAME[0], GAME[1], "setoption name KeepTree value maybe",
                     "setoption name KeepTree value true", GAME[2], "go nodes 20"], s)
    assert "info string setoption: KeepTree must be true or false" in out and not [c for c in s.log if c[0] == "advance"]
