"""The tools of match play against an outside opponent (-m gpu): tools/play_uci.py against the stub UCI engine, in a fresh process
(the tool starts its UCI processes before it opens the GPU), and tools/external_rate.py at a small size."""
import json
import os
import re
import subprocess
import sys

import pytest

import external_ref as xr
from helpers import san_to_move
from support import ROOT, run_torch_child, scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu

SALT_A, SALT_B = 0x1111, 0x2222
SEARCH = dict(rollout_num=8, cpuct=1.5, temperature=0.0, temperature_switch=0)

# runs a tool's main() in this (fresh) process and reports its exit status and output
CHILD = """
import contextlib, io, json, runpy, sys
tool, args = sys.argv[1], sys.argv[2:]
sys.argv = [tool] + args
out, code = io.StringIO(), 0
with contextlib.redirect_stdout(out):
    try:
        runpy.run_path(tool, run_name="__main__")
    except SystemExit as e:
        code = e.code if isinstance(e.code, int) else (1 if e.code else 0)
print(json.dumps({"code": code, "stdout": out.getvalue()}))
"""


def _result(outcome):
    return "unfinished" if outcome is None else "draw" if outcome["winner"] is None else outcome["winner"]


def test_play_uci_against_the_stub(scamd, orc, tmp_path):
    import scamd.san
    import scamd.traces
    games = {}
    for k in range(2):   # --swap: the engine is White in the first game, Black in the second
        w, b = (SALT_A, SALT_B) if k == 0 else (SALT_B, SALT_A)
        games[k] = orc.match_game(user_white=w, user_black=b, seed=3, game_id=k, num_steps=200, **SEARCH)
    keyed = xr.script_table(orc, {k: g["steps"] for k, g in games.items()}, 1)
    table = {line: mv for (_k, line), mv in keyed.items()}
    assert len(table) == len(keyed)   # (no position is answered differently in the two games)
    (tmp_path / "table.json").write_text(json.dumps(table))
    pgn, pattern = tmp_path / "match.pgn", str(tmp_path / "trace_{}.json")
    r = run_torch_child(tmp_path, CHILD, os.path.join(ROOT, "tools", "play_uci.py"), "--white-device", "cuda", "--black-type", "stockfish",
                        "--stockfish-bin", sys.executable, "--stockfish-arg", os.path.join(ROOT, "tests", "uci_stub.py"), "--stockfish-arg=--table",
                        "--stockfish-arg", str(tmp_path / "table.json"), "--stockfish-level", "3", "-r", "8", "--cpuct", "1.5",
                        "--temperature", "0", "--temperature-switch", "0", "--seed", "3", "--evaluator", "synth", "--salt", hex(SALT_A),
                        "--games", "2", "--concurrency", "2", "--swap", "--procs", "2", "--pgn", str(pgn), "-o", pattern, timeout=120)
    assert r["code"] == 0, r
    paths = [pattern.replace("{}", str(k + 1)) for k in range(2)]
    tr = scamd.traces.read(paths).check(paths)
    assert list(tr.n_steps) == [len(games[k]["steps"]) for k in range(2)]
    moves = [[s[0] for s in g] for g in tr.games()]
    assert moves == [[s[0] for s in games[k]["steps"]] for k in range(2)]
    for k in range(2):
        js = json.load(open(paths[k]))
        assert js["outcome"] == games[k]["outcome"]
        assert [tuple(s[:2]) + ([tuple(c) for c in s[2]],) for s in js["steps"]] == xr.expected_steps(games[k]["steps"], 1, k), k
    movetexts, winners = scamd.san.read_pgn(str(pgn))
    assert len(movetexts) == 2
    for k, mt in enumerate(movetexts):
        st, back = orc.State(), []
        for tok in scamd.san.tokenize(mt):
            m, _check, _mate = san_to_move(st, scamd.san.token_text(tok), orc)
            st.push(m)
            back.append(orc.uci(m))
        assert back == moves[k], k
    text = pgn.read_text()
    assert text.count('[White "synth-0x1111"]') == 1 and text.count('[Black "synth-0x1111"]') == 1 and "-level3" in text
    want = {key: dict.fromkeys(("White", "Black", "draw", "unfinished"), 0) for key in (0, 1)}
    for k in range(2):
        want[k][_result(games[k]["outcome"])] += 1
    m = re.search(r"games 2 slots 2 as-white: white-wins (\d+) black-wins (\d+) draws (\d+) unfinished (\d+)  as-black: white-wins (\d+) "
                  r"black-wins (\d+) draws (\d+) unfinished (\d+)   \(elo\.py input: 2/(\d+)/(\d+)\)", r["stdout"])
    assert m, r["stdout"]
    t = [int(x) for x in m.groups()]
    assert t[0:4] == list(want[0].values()) and t[4:8] == list(want[1].values())
    assert t[8] == t[0] + t[5] and t[9] == t[1] + t[4]


def test_external_rate_prints_its_lines():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "external_rate.py"), "--slots", "8", "--rollout", "4", "--plies", "2,6",
                        "--reps", "1", "--out", os.devnull], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines()]
    print(r.stdout)
    assert [ln["ply"] for ln in lines] == [2, 6]
    for ln in lines:
        assert set(ln) == {"tool", "host", "date", "slots", "rollout", "ply", "n_moves", "rounds", "round_ms", "wait_ms", "opponent_ms", "push_ms",
                           "set_position_ms", "x_set_position_over_round", "search_ply_ms", "round_share_of_ply", "error_flags"}
        assert ln["tool"] == "external_rate" and ln["slots"] == 8 and ln["rollout"] == 4 and ln["n_moves"] == 8 and ln["error_flags"] == 0
        for k in ("round_ms", "wait_ms", "opponent_ms", "push_ms", "set_position_ms", "search_ply_ms"):
            med, lo, hi = ln[k]
            assert 0 < lo <= med <= hi, (k, ln[k])
        assert ln["round_share_of_ply"] > 0 and ln["x_set_position_over_round"] > 0
