"""GPU (-m gpu): the engine behind UCI (tools/uci_engine.py) as a child process -- scripted stdin, every read under a deadline --
against the oracle's search and tests/report_ref.py; the project's own UciOpponent with this engine as its command inside
play_external; and tools/report_rate.py at a small size."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import pytest

import deep_lines as dl
import lines
import report_ref as rr
from support import ROOT, run_torch_child, scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu

TOOL = os.path.join(ROOT, "tools", "uci_engine.py")
SALT = 0x2222
START = 90.0   # seconds for the child to import the package and open the GPU
REPLY = 30.0


def _salt(s):
    box = C.c_uint64(s)
    return box, C.cast(C.byref(box), C.c_void_p)


def _oracle_lines(orc, st, sims, cpuct, multipv, salt=None, evaluator="synth"):
    """report_ref's lines of the oracle's search from `st`"""
    box, user = _salt(salt) if salt is not None else (None, None)
    srch = orc.Search(st)
    for _ in range(sims):
        srch.sim(evaluator=dl.EVALUATORS[evaluator], user=user, cpuct=cpuct, with_noise=False)
    return rr.report(srch.dump(), rr.WHITE if st.turn else rr.BLACK, multipv, 64)["lines"]


def _go(pr, command, timeout=REPLY):
    """send a `go`, read to its bestmove -> (the last info line per multipv rank as dicts, the bestmove)"""
    pr.send(command)
    deadline = time.monotonic() + timeout
    info = {}
    while True:
        words = pr.readline(deadline).split()
        if words[:1] == ["bestmove"]:
            return [info[k] for k in sorted(info)], words[1]
        if words[:2] == ["info", "depth"]:
            f = dict(zip(words[1:13:2], words[2:13:2]))   # depth multipv nodes nps time score
            i = words.index("score")
            info[int(f["multipv"])] = dict(depth=int(f["depth"]), nodes=int(f["nodes"]), score=(words[i + 1], int(words[i + 2])),
                                           pv=words[words.index("pv") + 1:])


def _same(info, ref, nodes):
    assert len(info) == len(ref)
    for got, x in zip(info, ref):
        assert (got["depth"], got["nodes"], got["score"], got["pv"]) == (ref[0]["len"], nodes, x["score"], x["pv"]), (got, x)


@pytest.fixture()
def engine(scamd):
    from scamd import external as ext
    procs = []

    def start(*args):
        pr = ext._UciProc([sys.executable, TOOL, *args])
        procs.append(pr)
        pr.send("uci")
        pr.wait_for("uciok", START)
        return pr

    yield start
    for pr in procs:
        if pr.p.poll() is None:
            pr.p.kill()
        pr.reap(time.monotonic() + 5)


def test_go_nodes_is_the_search_and_stop_and_quit(scamd, orc, engine):
    pr = engine("--evaluator", "synth", "--salt", hex(SALT))
    pr.send("setoption name MultiPV value 3")
    pr.send("position startpos moves " + " ".join(lines.WIDE))
    info, best = _go(pr, "go nodes 60")
    ref = _oracle_lines(orc, lines.pushed(orc, lines.WIDE), 60, 2.5, 3, SALT)
    _same(info, ref, 60)
    assert best == ref[0]["move"]
    # ... from a FEN, with another cpuct; the same search again gives the same answer (every go starts from a fresh tree)
    pr.send("setoption name CPuct value 1.5")
    pr.send("position fen " + dl.COMB_B)
    ref = _oracle_lines(orc, orc.State(dl.COMB_B), 60, 1.5, 3, SALT)
    for _ in range(2):
        info, best = _go(pr, "go nodes 60")
        _same(info, ref, 60)
        assert best == ref[0]["move"] and len(info) == 2
    # ... moves behind the FEN reach the handle
    pr.send("position fen " + dl.COMB_B + " moves a8b8 h1g1")
    st = orc.State(dl.COMB_B)
    st.push("a8b8")
    st.push("h1g1")
    info, best = _go(pr, "go nodes 40")
    _same(info, _oracle_lines(orc, st, 40, 1.5, 3, SALT), 40)
    # no legal move
    pr.send("position startpos moves " + " ".join(lines.MATED))
    assert _go(pr, "go nodes 20") == ([], "0000")
    # go infinite answers when it is told to stop
    pr.send("position startpos")
    pr.send("go infinite")
    pr.wait_for("info", REPLY)
    pr.send("isready")
    pr.wait_for("readyok", REPLY)
    pr.send("stop")
    words = pr.wait_for("bestmove", REPLY).split()
    assert len(words) == 2 and len(words[1]) == 4
    pr.send("quit")
    assert pr.p.wait(timeout=REPLY) == 0


def test_go_nodes_with_a_network_is_sc_search(scamd, engine):
    eng = scamd.Engine(1, 128, seed=2)
    root_q, kids = scamd.search(eng, lines.WIDE, 60, cpuct=2.5, noise=False)
    eng.close()
    order = sorted(range(len(kids)), key=lambda i: (-kids[i][1], i))
    pr = engine("--blocks", "1", "--channels", "128", "--net-seed", "2")
    pr.send("setoption name MultiPV value 5")
    pr.send("position startpos moves " + " ".join(lines.WIDE))
    info, best = _go(pr, "go nodes 60")
    assert best == kids[order[0]][0] and [x["pv"][0] for x in info] == [kids[i][0] for i in order[:5]]
    assert all(x["nodes"] == 60 for x in info)
    from scamd import report as rp
    for x, i in zip(info, order):
        if x["score"][0] == "cp":
            assert x["score"][1] == rp.centipawns(rp.line_q(kids[i][2], kids[i][1], rr.WHITE))
    pr.send("quit")
    assert pr.p.wait(timeout=REPLY) == 0


_MATCH_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
from scamd import external as ext      # (loads no library and opens no device)
# the pool first: UciOpponent starts its processes before this process opens the GPU
opp = ext.UciOpponent([sys.executable, sys.argv[2], "--evaluator", "synth", "--salt", sys.argv[3]], n_procs=1, options={"CPuct": 1.5},
                      go="nodes 8", position="moves", timeout=90.0)
try:
    res = ext.play_external(None, opp, n_games=2, concurrency=2, rollout=8, cpuct=1.5, num_steps=12, seed=3, colours=1, evaluator="synth",
                            salt=int(sys.argv[4], 0))
finally:
    opp.close()
print(json.dumps({"moves": [[s[0] for s in t["steps"]] for t in res["traces"]], "total": res["total"]}))
"""


def test_uci_opponent_drives_the_engine(scamd, orc, tmp_path):
    """2 games on 2 slots, rollout 8, the opponent one process of this engine (with the test process and the match's own: three
    processes hold the GPU): every ply the opponent played is the first most-visited child of the search from that move list"""
    out = run_torch_child(tmp_path, _MATCH_CHILD, os.path.join(ROOT, "smart-chess-rust_amd"), TOOL, hex(SALT), hex(0x1111), timeout=300)
    assert out["total"] == 2 and all(len(m) >= 4 for m in out["moves"])
    checked = 0
    for g, moves in enumerate(out["moves"]):
        for ply, mv in enumerate(moves):
            if ply % 2 == g % 2:
                continue   # colours 1: the engine of the match is White in game 0 and Black in game 1; the opponent plays the other plies
            ref = _oracle_lines(orc, lines.pushed(orc, moves[:ply]), 8, 1.5, 1, SALT)
            assert mv == ref[0]["move"], (g, ply, mv, ref[0])
            checked += 1
    assert checked >= 4


def test_report_rate_prints_its_lines():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "report_rate.py"), "--slots", "8", "--rollout", "8", "--reps", "1", "--out", os.devnull],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [json.loads(ln) for ln in r.stdout.splitlines()]
    print(r.stdout)
    assert [ln["multipv"] for ln in out] == [1, 8]
    for ln in out:
        assert set(ln) == {"tool", "host", "date", "slots", "rollout", "multipv", "pv_cap", "reps", "nodes_per_slot", "mean_pv_len", "call_ms", "device_ms",
                           "total_ms", "tree_ms", "search_ply_ms", "x_tree_over_report", "report_share_of_ply", "same_moves", "error_flags"}
        assert ln["tool"] == "report_rate" and ln["slots"] == 8 and ln["rollout"] == 8 and ln["error_flags"] == 0 and ln["same_moves"] is True
        for k in ("call_ms", "device_ms", "total_ms", "tree_ms", "search_ply_ms"):
            med, lo, hi = ln[k]
            assert 0 < lo <= med <= hi, (k, ln[k])
        assert ln["x_tree_over_report"] > 0 and ln["report_share_of_ply"] > 0
