"""CPU: the search report's rules as tests/report_ref.py states them -- on hand-built trees whose answers are written out here, on
the oracle's trees (properties that do not depend on how the report is computed), against deliberately wrong rules, each of which
must give a different report on at least one of these trees -- and the UCI protocol class (scamd.uci.Protocol) over a stub searcher:
parsing, the time allocation, the info and bestmove lines, stop, quit and the node clamp.  No device is needed."""
import queue

import numpy as np
import pytest

import deep_lines as dl
import lines
import report_ref as rr
from report_ref import BLACK, WHITE, StubSearcher, make_tree

SIMS = 200


def mv(i):
    return (i % 64) | ((i * 7 + 9) % 64) << 6


# root 0 with four children 1..4 (N 3, 3, 0, 3); 1 has children 5, 6 (N 1, 1), 2 has child 7, 5 has the unvisited children 8, 9
HAND = make_tree([(10, 1.0, 0, 1, 4),
                  (3, 1.5, mv(1), 5, 2), (3, 0.5, mv(2), 7, 1), (0, 0.0, mv(3), -1, 0), (3, 3.0, mv(4), -3, 0),
                  (1, 0.5, mv(5), 8, 2), (1, 0.0, mv(6), -2, 0), (2, -2.0, mv(7), -4, 0), (0, 0.0, mv(8), -1, 0), (0, 0.0, mv(9), -1, 0)])


def chain(visited):
    """a root and a one-child chain below it: nodes 1 .. visited have visits, node visited + 1 has none"""
    L = visited + 1
    return make_tree([(L - i, 0.25 * (L - i), mv(i), i + 1 if i < L else -1, 1 if i < L else 0) for i in range(L + 1)])


def test_hand_built_ranks_walks_and_scores():
    r = rr.report(HAND, WHITE, multipv=224, pv_cap=64)
    assert (r["n_lines"], r["n_root_children"], r["root_children_n"], r["root_n"], float(r["root_w"])) == (4, 4, 9, 10, 1.0)
    ln = r["lines"]
    assert [x["child"] for x in ln] == [0, 1, 3, 2]                       # visits descending, ties in the generator's order, N == 0 last
    assert [x["n"] for x in ln] == [3, 3, 3, 0]
    assert [(x["len"], x["end"]) for x in ln] == [(2, rr.END_OPEN), (2, rr.END_BLACK_WON), (1, rr.END_WHITE_WON), (1, rr.END_OPEN)]
    assert ln[0]["moves"] == [mv(1), mv(5)]                               # the tie below goes to the lower index; 5's children have no visit
    assert ln[1]["moves"] == [mv(2), mv(7)] and ln[3]["moves"] == [mv(3)]
    assert [x["score"] for x in ln] == [("cp", rr.centipawns(0.5)), ("mate", -1), ("mate", 1), ("cp", 0)]
    assert [x["q"] for x in ln] == [0.5, float(np.float32(0.5) / np.float32(3)), 1.0, 0.0]
    assert rr.report(HAND, WHITE, multipv=2)["n_lines"] == 2 and rr.report(HAND, WHITE, live=False)["n_lines"] == 0
    # Black to move at the root: q changes its sign, the mate scores follow the length alone
    b = rr.report(HAND, BLACK, multipv=224)["lines"]
    assert [x["q"] for x in b] == [-x["q"] if x["n"] else 0.0 for x in ln] and [x["score"] for x in b][1:3] == [("mate", -1), ("mate", 1)]
    # pv_cap cuts the moves, not the length
    assert [(x["len"], x["moves"]) for x in rr.report(HAND, WHITE, multipv=2, pv_cap=1)["lines"]] == [(2, [mv(1)]), (2, [mv(2)])]
    assert [(x["len"], x["moves"]) for x in rr.report(HAND, WHITE, multipv=1, pv_cap=0)["lines"]] == [(2, [])]


def test_hand_built_edges():
    assert rr.report(make_tree([(0, 0.0, 0, -1, 0)]), WHITE)["n_lines"] == 0                      # a fresh root
    for fc, w in ((-2, 0.0), (-3, 1.0), (-4, -1.0), (-1, -1.0)):                                 # a root without a legal move
        r = rr.report(make_tree([(5, 5 * w, 0, fc, 0)]), WHITE)
        assert (r["n_lines"], r["n_root_children"], r["root_n"]) == (0, 0, 5)
    assert rr.report(dict(n=np.zeros(0, np.int32), q=np.zeros(0, np.float32)), WHITE)["n_lines"] == 0
    one = rr.report(chain(5), WHITE)["lines"]
    assert len(one) == 1 and one[0]["len"] == 5 and one[0]["end"] == rr.END_OPEN and one[0]["moves"] == [mv(i) for i in range(1, 6)]
    # the oracle's form of a terminal: first_child stays -1, the node is visited and childless, its value says who won
    t = make_tree([(4, -3.0, 0, 1, 1), (3, -3.0, mv(1), -1, 0)])
    assert [(x["len"], x["end"], x["score"]) for x in rr.report(t, BLACK)["lines"]] == [(1, rr.END_BLACK_WON, ("mate", 1))]
    t["q"][1] = 0.0
    assert rr.report(t, BLACK)["lines"][0]["end"] == rr.END_DRAW


@pytest.mark.parametrize("visited,want", [(70, (70, rr.END_OPEN)), (1023, (1023, rr.END_OPEN)), (1024, (1024, rr.END_OPEN)),
                                          (1025, (1024, rr.END_DEPTH)), (1100, (1024, rr.END_DEPTH))])
def test_walk_limit(visited, want):
    x = rr.report(chain(visited), WHITE, pv_cap=1024)["lines"][0]
    assert (x["len"], x["end"]) == want and len(x["moves"]) == want[0]
    assert len(rr.report(chain(visited), WHITE, pv_cap=64)["lines"][0]["moves"]) == 64


def test_scores():
    assert rr.centipawns(0.0) == 0 and rr.centipawns(1.0) == rr.centipawns(0.9999) == round(400 * np.log10(999))
    assert rr.centipawns(-1.0) == -rr.centipawns(1.0) and rr.centipawns(0.5) == round(400 * np.log10(3)) == 191
    assert [rr.score(0.3, n, rr.END_WHITE_WON) for n in (1, 2, 3, 4, 5)] == [("mate", 1), ("mate", -1), ("mate", 2), ("mate", -2), ("mate", 3)]
    assert rr.score(0.3, 3, rr.END_DRAW) == rr.score(0.3, 3, rr.END_OPEN) == rr.score(0.3, 3, rr.END_DEPTH) == ("cp", rr.centipawns(0.3))
    # the package's own functions are the same ones
    from scamd import report as rep
    for q in (-1.0, -0.37, 0.0, 1e-3, 0.5, 0.9999, 1.0):
        assert rep.centipawns(q) == rr.centipawns(q)
        for n in range(1, 7):
            for end in range(5):
                assert rep.line_score(q, n, end) == rr.score(q, n, end)
    for w, n, turn in ((1.5, 3, WHITE), (1.5, 3, BLACK), (-7.0, 9, BLACK), (0.0, 0, BLACK)):
        assert np.float32(rep.line_q(np.float32(w), n, turn)).tobytes() == np.float32(rr.line_q(w, n, turn)).tobytes()


# ------------------------------------------------------------------ the oracle's trees
@pytest.fixture(scope="module")
def oracle_trees(orc):
    """name -> (tree, side to move at the root) after SIMS simulations of the oracle's search"""
    out = {}
    starts = {"start": orc.State(), "wide": lines.pushed(orc, lines.WIDE), "wide137": lines.pushed(orc, lines.WIDE137)}
    starts.update({k: orc.State(f) for k, f in dl.POSITIONS.items()})
    for name, st in starts.items():
        for ev in ("synth", "synth_uniform"):
            srch = orc.Search(st)
            for _ in range(SIMS):
                srch.sim(evaluator=dl.EVALUATORS[ev], cpuct=2.5, with_noise=False)
            out[name, ev] = (srch.dump(), WHITE if st.turn else BLACK)
    return out


def test_oracle_trees_properties(oracle_trees):
    for key, (t, turn) in oracle_trees.items():
        r = rr.report(t, turn, multipv=224, pv_cap=1024)
        fc, nc = int(t["first_child"][0]), int(t["n_child"][0])
        assert r["n_lines"] == nc == r["n_root_children"] and r["root_children_n"] == SIMS - 1 and r["root_n"] == SIMS, key
        assert sorted(x["child"] for x in r["lines"]) == list(range(nc)), key
        ns = [x["n"] for x in r["lines"]]
        assert ns == sorted(ns, reverse=True) and r["lines"][0]["child"] == int(np.argmax(t["n"][fc:fc + nc])), key
        for a, b in zip(r["lines"], r["lines"][1:]):
            assert a["n"] > b["n"] or a["child"] < b["child"], key
        for x in r["lines"]:
            nodes, end = rr.walk(t, fc + x["child"])
            assert len(nodes) == x["len"] and [int(t["move"][y]) for y in nodes] == x["moves"], key
            for y, z in zip(nodes, nodes[1:]):
                sib = t["n"][t["first_child"][y]:t["first_child"][y] + t["n_child"][y]]
                assert t["parent"][z] == y and t["n"][z] == sib.max() > 0 and z == t["first_child"][y] + int(np.argmax(sib)), key
            last = nodes[-1]
            if t["n_child"][last]:
                assert end == rr.END_OPEN and t["n"][t["first_child"][last]:t["first_child"][last] + t["n_child"][last]].max() == 0, key
            elif t["n"][last]:
                assert end in (rr.END_DRAW, rr.END_WHITE_WON, rr.END_BLACK_WON), key
            else:
                assert end == rr.END_OPEN and x["len"] == 1 or t["n"][last] == 0, key
    for ev in ("synth", "synth_uniform"):
        # a forced line after s simulations is a chain of s + 1 nodes whose last has no visit: one line of s - 1 moves
        for name in dl.FORCED:
            (x,) = rr.report(*oracle_trees[name, ev], multipv=224, pv_cap=1024)["lines"]
            assert (x["len"], x["end"], x["n"]) == (SIMS - 1, rr.END_OPEN, SIMS - 1), (name, ev)
        (x,) = rr.report(*oracle_trees["sink", ev], multipv=224)["lines"]     # White's only move stalemates Black
        assert (x["len"], x["end"], x["score"], x["pv"]) == (1, rr.END_DRAW, ("cp", 0), ["h1g1"]), ev
        assert rr.report(*oracle_trees["wide137", ev], multipv=224)["n_lines"] == 137


WRONG = {"last-maximum ties": dict(tie="last"), "a walk that follows an unvisited child": dict(follow_unvisited=True),
         "ranks by W": dict(rank_by="w"), "a walk that stops at 64": dict(walk_limit=64), "q without the Black flip": dict(black_flip=False),
         "mate sign by the value": dict(mate_sign="value")}


def _summary(r):
    return [(x["child"], x["len"], x["end"], tuple(x["moves"]), x["q"], x["score"]) for x in r["lines"]]


@pytest.mark.parametrize("name", list(WRONG))
def test_wrong_rules_are_told_apart(oracle_trees, name):
    """every wrong rule changes the report of at least one tree -- and the names of those trees are printed"""
    trees = {("hand", t): (HAND, t) for t in (WHITE, BLACK)}
    trees[("chain", 1100)] = (chain(1100), WHITE)
    trees.update(oracle_trees)
    rules = dict(rr.RIGHT, **WRONG[name])
    differ = [k for k, (t, turn) in trees.items()
              if _summary(rr.report(t, turn, 224, 1024)) != _summary(rr.report(t, turn, 224, 1024, rules=rules))]
    print(name, "->", differ)
    assert differ, name
    if name in ("last-maximum ties", "ranks by W", "a walk that stops at 64", "q without the Black flip"):
        assert any(k in oracle_trees for k in differ), (name, differ)   # ... on a tree of a real search too


# ------------------------------------------------------------------ the protocol class over a stub searcher
def _serve(commands, searcher=None, clock=None):
    from scamd import uci
    s = searcher or StubSearcher()
    out = []
    q = queue.Queue()
    for c in commands:
        q.put(c)
    q.put(None)
    p = uci.Protocol(s, out.append, **({"clock": clock} if clock else {}))
    assert p.run(q) == 0
    return out, s, p


def test_uci_handshake_and_options():
    out, s, p = _serve(["uci", "isready", "setoption name MultiPV value 3", "setoption name cpuct value 1.5", "setoption name Chunk value 16",
                        "setoption name InfoEvery value 0", "setoption name Hash value 1", "setoption name MultiPV value 0", "ucinewgame", "bogus"])
    assert out[0].startswith("id name ") and out[1].startswith("id author ") and out[-4:-2] == ["uciok", "readyok"]
    opts = [ln for ln in out if ln.startswith("option name ")]
    assert [ln.split()[2] for ln in opts] == ["MultiPV", "CPuct", "Chunk", "InfoEvery"]
    assert "option name MultiPV type spin default 1 min 1 max 224" in opts and "option name Chunk type spin default 64 min 1 max 4096" in opts
    assert p.opt == {"MultiPV": 3, "CPuct": 1.5, "Chunk": 16, "InfoEvery": 0}
    assert out[-2] == "info string setoption: no option 'Hash'" and out[-1].startswith("info string setoption: MultiPV must lie in")
    assert s.calls == ["new_game", "close"]


def test_position_and_go_parsing():
    from scamd import uci
    assert uci.parse_position(["startpos"]) == (None, [])
    assert uci.parse_position("startpos moves e2e4 e7e5 a7a8q".split()) == (None, ["e2e4", "e7e5", "a7a8q"])
    assert uci.parse_position(("fen " + dl.SINK + " moves h1g1").split()) == (dl.SINK, ["h1g1"])
    assert uci.parse_position("fen 8/8/8/8/8/8/8/K1k5 w - -".split()) == ("8/8/8/8/8/8/8/K1k5 w - -", [])
    for bad in ("", "fen 8/8 w", "startpos moves e2e9", "startpos e2e4", "start"):
        with pytest.raises(ValueError):
            uci.parse_position(bad.split())
    assert uci.parse_go("nodes 60".split()) == {"nodes": 60} and uci.parse_go(["infinite"]) == {"infinite": True}
    assert uci.parse_go("wtime 60000 btime 50000 winc 1000 binc 2000 movestogo 12 ponder".split()) == dict(wtime=60000, btime=50000, winc=1000, binc=2000,
                                                                                                         movestogo=12)
    with pytest.raises(ValueError):
        uci.parse_go("nodes many".split())
    out, s, p = _serve(["position fen " + dl.FORCED_B + " moves a8b8", "position startpos moves e2e9"])
    assert s.position == (dl.FORCED_B, ["a8b8"]) and not p.black_to_move and out == ["info string position: 'e2e9' is not a UCI move"]


def test_time_allocation():
    from scamd import uci
    for f in (uci.allocate_ms, rr.allocate_ms):
        assert f(60000, 0, 0) == 2000 and f(60000, 1000, 0) == 2500 and f(60000, 0, 40) == 1500 and f(60000, 0, 5) == 2000
        assert f(1000, 5000, 0) == 500 and f(0, 0, 0) == 0 and f(300, 0, 1) == 10
    # the side to move takes its own clock; the clock ends the search between two chunks
    now = [0.0]

    def tick(s):
        now[0] += 0.4

    out, s, _ = _serve(["position startpos moves e2e4", "go wtime 900000 btime 60000 binc 1000"], StubSearcher(on_run=tick), clock=lambda: now[0])
    assert sum(s.runs) == 64 * 7 and out[-1] == "bestmove e2e4"          # 2500 ms: over after the seventh chunk of 0.4 s
    out, s, _ = _serve(["go movetime 1000"], StubSearcher(on_run=tick), clock=lambda: now[0])
    assert sum(s.runs) == 64 * 3


def test_go_nodes_info_and_bestmove_lines():
    out, s, _ = _serve(["setoption name MultiPV value 2", "setoption name InfoEvery value 0", "position startpos", "go nodes 100"], clock=lambda: 2.0)
    assert s.runs == [64, 36] and s.cpuct == 2.5
    assert out == ["info depth 2 multipv 1 nodes 64 nps 0 time 0 score cp 30 pv e2e4 e7e5", "info depth 2 multipv 2 nodes 64 nps 0 time 0 score cp 20 pv d2d4",
                   "info depth 2 multipv 1 nodes 100 nps 0 time 0 score cp 30 pv e2e4 e7e5", "info depth 2 multipv 2 nodes 100 nps 0 time 0 score cp 20 pv d2d4",
                   "bestmove e2e4"]
    now = [0.0]

    def tick(s):
        now[0] += 0.25

    out, s, _ = _serve(["go nodes 128"], StubSearcher(mate=-3, on_run=tick), clock=lambda: now[0])
    assert out == ["info depth 2 multipv 1 nodes 64 nps 256 time 250 score mate -3 pv e2e4 e7e5",          # InfoEvery 500: one line on the way
                   "info depth 2 multipv 1 nodes 128 nps 256 time 500 score mate -3 pv e2e4 e7e5", "bestmove e2e4"]
    out, _, _ = _serve(["go nodes 10"], StubSearcher(moves=()))
    assert out == ["bestmove 0000"]                                                                         # no legal move


def test_go_nodes_is_clamped():
    out, s, _ = _serve(["setoption name Chunk value 4096", "go nodes 1000000"])
    assert sum(s.runs) == 59999 and max(s.runs) == 4096 and out[-1] == "bestmove e2e4"
    out, s, _ = _serve(["setoption name Chunk value 4096", "go nodes 59999"])
    assert sum(s.runs) == 59999


def test_stop_during_go_infinite():
    from scamd import uci
    q, out = queue.Queue(), []

    def post(s):
        if len(s.runs) == 4:   # at the start of the fifth chunk
            for c in ("isready", "stop", "isready", "quit"):
                q.put(c)

    s = StubSearcher(on_run=post)
    p = uci.Protocol(s, out.append)
    q.put("position startpos")
    q.put("go infinite")
    assert p.run(q) == 0
    # the fifth chunk's look at the queue answers `isready` and ends the search; what follows `stop` is served after `bestmove`
    assert len(s.runs) == 5 and out[-4] == "readyok" and out[-3].startswith("info depth 2 multipv 1 nodes 320 ")
    assert out[-2:] == ["bestmove e2e4", "readyok"] and s.calls[-1] == "close"
    # a search that has used its node pool waits for `stop` before it answers; a `stop` that is waiting is seen after the first chunk
    out, s, _ = _serve(["setoption name Chunk value 4096", "go infinite", "stop"])
    assert s.runs == [4096] and out[-1] == "bestmove e2e4"
    out, s, _ = _serve(["setoption name Chunk value 4096", "go infinite"])     # (the end of input ends it too)
    assert sum(s.runs) == 59999 and out[-1] == "bestmove e2e4"


def test_commands_behind_a_search_wait_for_it():
    out, s, _ = _serve(["go nodes 200", "position startpos moves e2e4", "go nodes 64", "stop"])
    assert [ln for ln in out if ln.startswith("bestmove")] == ["bestmove e2e4"] * 2 and s.position == (None, ["e2e4"])
    assert "nodes 200 " in out[out.index("bestmove e2e4") - 1] and "nodes 64 " in out[-2]     # both ran to their limits


@pytest.mark.parametrize("script", [["quit"], ["uci", "quit", "isready"], ["go infinite", "quit"], ["go nodes 1000", "quit", "go nodes 5"],
                                    ["position startpos", "go infinite"]])
def test_quit_at_any_point(script):
    out, s, p = _serve(script)
    assert s.calls[-1] == "close" and "readyok" not in out
    if "go" in " ".join(script):
        assert out[-1] == "bestmove e2e4" and len([ln for ln in out if ln.startswith("bestmove")]) == 1


def test_error_flags_answer_from_the_last_clean_report():
    out, s, _ = _serve(["go nodes 1000"], StubSearcher(flags_at=200))
    assert s.runs == [64, 64, 64, 64]
    assert out[-3].startswith("info string search error flags 8") and out[-2].startswith("info depth 2 multipv 1 nodes 192 ") and out[-1] == "bestmove e2e4"
    out, _, _ = _serve(["go nodes 1000"], StubSearcher(flags_at=1))
    assert out[-2].startswith("info string search error flags 8") and out[-1] == "bestmove 0000"
