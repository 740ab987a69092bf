"""Outside opponents, the checks that need no GPU: the UCI process pool of scamd.external against a stub engine (tests/uci_stub.py),
the scripted opponent, and the position lines both send."""
import glob
import importlib
import json
import os
import sys
import time

import pytest

import external_ref as xr
from support import ROOT, scamd_built  # noqa: F401

STUB = os.path.join(ROOT, "tests", "uci_stub.py")
START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
AFTER_E4 = "rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq - 0 1"


@pytest.fixture(scope="module")
def ext(scamd):
    return importlib.import_module("scamd.external")


def _req(game, fen, moves=(), slot=None, ply=None):
    return dict(slot=game if slot is None else slot, game=game, ply=len(moves) if ply is None else ply, fen=fen, moves=list(moves))


def _stub(tmp_path, table, *flags):
    path = tmp_path / "table.json"
    path.write_text(json.dumps(table))
    return [sys.executable, STUB, "--table", str(path), "--log", str(tmp_path / "log.txt"), *flags]


def _logs(tmp_path):
    return [open(p).read().splitlines() for p in sorted(glob.glob(str(tmp_path / "log.*.txt")))]


def _alive(pids):
    out = []
    for pid in pids:
        try:
            os.kill(pid, 0)
            out.append(pid)
        except OSError:
            pass
    return out


def test_position_lines(ext):
    r = _req(3, AFTER_E4, ["e2e4"])
    assert ext.position_line(r) == "position fen " + AFTER_E4
    assert ext.position_line(r, "moves") == "position startpos moves e2e4"
    assert ext.position_line(_req(0, START), "moves") == "position startpos"
    with pytest.raises(ValueError):
        ext.position_line(r, "pgn")


def test_scripted_opponent(ext, scamd):
    line = "position fen " + START
    opp = ext.ScriptedOpponent({line: "e2e4", (1, line): "d2d4", "position fen " + AFTER_E4: "c7c5"})
    assert not opp.needs_moves
    assert opp.moves([_req(0, START), _req(1, START), _req(2, AFTER_E4, ["e2e4"])]) == ["e2e4", "d2d4", "c7c5"]
    assert opp.moves([]) == []
    with pytest.raises(scamd.EngineError, match="game 7"):
        opp.moves([_req(7, "8/8/8/8/8/8/8/K1k5 w - - 0 1")])
    by_moves = ext.ScriptedOpponent({"position startpos moves e2e4": "e7e5"}, position="moves")
    assert by_moves.needs_moves and by_moves.moves([_req(0, AFTER_E4, ["e2e4"])]) == ["e7e5"]


def test_script_table_replays_the_other_side(ext, orc):
    """the helper of the GPU tests: a table made from a game answers every opponent ply of it, in both position forms"""
    game = orc.match_game(user_white=1, user_black=2, seed=4, game_id=9, num_steps=12, rollout_num=8)
    for form in ("fen", "moves"):
        opp = ext.ScriptedOpponent(xr.script_table(orc, {5: game["steps"]}, 0, form), position=form)
        st, played = orc.State(), []
        for i, (move, _q, _kids) in enumerate(game["steps"]):
            if i % 2 == 1:
                assert opp.moves([_req(5, st.fen(), played)]) == [move], (form, i)
            st.push(move)
            played.append(move)
    assert xr.expected_steps(game["steps"], 0, 5)[0] == game["steps"][0]
    move, _q, kids = game["steps"][1]
    assert xr.expected_steps(game["steps"], 0, 5)[1] == (move, 0.0, [(m, int(m == move), 0.0, 0.0) for m, *_ in kids])
    assert xr.expected_steps(game["steps"], 2, 5)[0] == xr.pushed_step(game["steps"][0])


def test_handshake_options_and_both_position_forms(ext, tmp_path):
    table = {"position fen " + START: "e2e4", "position startpos moves e2e4": "e7e5"}
    with ext.UciOpponent(_stub(tmp_path, table), n_procs=1, options={"Skill Level": 3, "Threads": 1}, go="depth 2") as opp:
        assert opp.moves([_req(0, START)]) == ["e2e4"]
        assert opp.moves([_req(0, START)]) == ["e2e4"]     # the same game: no second ucinewgame
        assert opp.moves([_req(1, START)]) == ["e2e4"]
    (log,) = _logs(tmp_path)
    assert log[:5] == ["uci", "setoption name Skill Level value 3", "setoption name Threads value 1", "isready", "ucinewgame"]
    assert log[5:] == ["position fen " + START, "go depth 2", "position fen " + START, "go depth 2", "ucinewgame",
                       "position fen " + START, "go depth 2", "quit"]
    for p in glob.glob(str(tmp_path / "log.*.txt")):
        os.remove(p)
    with ext.UciOpponent(_stub(tmp_path, table), n_procs=1, position="moves") as opp:
        assert opp.needs_moves and opp.moves([_req(0, AFTER_E4, ["e2e4"])]) == ["e7e5"]
    (log,) = _logs(tmp_path)
    assert log[-3:] == ["position startpos moves e2e4", "go depth 1", "quit"]


def test_requests_are_dealt_over_the_processes_and_replies_keep_their_order(ext, tmp_path):
    fens = [f"8/8/8/8/8/8/8/K1k5 w - - {i} 1" for i in range(8)]
    table = {"position fen " + f: f"a1a{2 + i % 2}" if i % 3 else "a1b1" for i, f in enumerate(fens)}
    opp = ext.UciOpponent(_stub(tmp_path, table), n_procs=3)
    pids = [pr.p.pid for pr in opp.procs]
    assert len(set(pids)) == 3 and _alive(pids) == pids
    reqs = [_req(i, f) for i, f in enumerate(fens)]
    assert opp.moves(reqs) == [table["position fen " + f] for f in fens]
    opp.close()
    assert _alive(pids) == [] and opp.procs == []
    opp.close()   # twice is fine
    served = sorted(sorted(ln[len("position fen "):] for ln in log if ln.startswith("position")) for log in _logs(tmp_path))
    assert served == sorted(sorted(fens[k::3]) for k in range(3))


@pytest.mark.parametrize("flags,why", [(("--delay", "30"), "within"), (("--die-after", "0"), "died"), (("--none",), r"\(none\)")],
                         ids=["timeout", "dead", "none"])
def test_failures_name_the_game(ext, scamd, tmp_path, flags, why):
    opp = ext.UciOpponent(_stub(tmp_path, {}, *flags), n_procs=2, timeout=0.5)
    pids = [pr.p.pid for pr in opp.procs]
    t0 = time.monotonic()
    with pytest.raises(scamd.EngineError, match=r"game 41: .*" + why):
        opp.moves([_req(41, START), _req(42, START)])
    assert time.monotonic() - t0 < 10
    opp.close()
    for _ in range(100):   # (a killed child is reaped by close(); give the kernel a moment)
        if not _alive(pids):
            break
        time.sleep(0.01)
    assert _alive(pids) == []


def test_a_missing_program_raises_and_leaves_nothing(ext, tmp_path):
    with pytest.raises(OSError):
        ext.UciOpponent([str(tmp_path / "no-such-engine")], n_procs=2)
    with pytest.raises(ValueError):
        ext.UciOpponent(_stub(tmp_path, {}), n_procs=9)
