"""Match play from opening lines (-m gpu): sc_selfplay_set_openings starts game k of a match handle from line k.  A game with a line of
length L is the CONTINUATION of the from-the-start game of the same id and seed whose first L moves were the line: the end-of-ply draw
is keyed by the absolute ply, the search tree is fresh at every ply.  So the reference of every case is a game from the start position
-- the CPU oracle's restatement of the `play` loop, or this engine's own one-game handle -- cut at L."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from support import ROOT, scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu

PLAY = os.path.join(ROOT, "smart-chess-rust_amd", "lib", "sc-play")
SALT_A, SALT_B = 11, 22
SEARCH = dict(rollout_num=20, cpuct=1.5, temperature=0.0, temperature_switch=0)
HANDLE = dict(seed=5, with_noise=False, outcome_gate=-1, tie_random=True, **SEARCH)
ORACLE = {"synth": "orc_eval_synth", "synth_coarse": "orc_eval_synth_coarse"}
KEYS = ("White", "Black", "draw", "unfinished")
ZERO = dict.fromkeys(KEYS, 0)


def _oracle_game(orc, evaluator, game_id, num_steps, white=SALT_A, black=SALT_B):
    ev = ORACLE[evaluator]
    return orc.match_game(white=ev, user_white=white, black=ev, user_black=black, num_steps=num_steps, seed=5, game_id=game_id, **SEARCH)


def _moves(game, n):
    return [s[0] for s in game["steps"][:n]]


def _match(scamd, lines, evaluator="synth", colours=0, salts=(SALT_A, SALT_B), **kw):
    """a synthetic match handle with `lines` (None: no sc_selfplay_set_openings call), not yet run"""
    sp = scamd.SelfPlay(None, evaluator=evaluator, **{**HANDLE, **kw})
    sp.set_match(None, None, salts[0], salts[1], colours=colours)
    if lines is not None:
        sp.set_openings(lines)
    return sp


def _finished(sp, n_games):
    st = sp.stats()
    assert st["error_flags"] == 0 and st["games_finished"] == n_games and st["games_active"] == 0, st
    return [sp.trace(k) for k in range(n_games)]


# ---------------------------------------------------------------------------------- 1. continuation, mixed parity, recycled slots
LENGTHS = [0, 1, 2, 3, 4, 7, 8]


@pytest.mark.parametrize("evaluator", ["synth", "synth_coarse"])
def test_games_continue_the_oracles_games(scamd, orc, evaluator):
    """7 games on 3 slots, a is White in all of them, lines of even and odd length: game k searches plies L_k .. L_k + 9 of the
    oracle's game k -- moves, root q, and every child's move, N, Q and uct bit for bit"""
    ref = [_oracle_game(orc, evaluator, k, 18) for k in range(7)]
    assert all(len(g["steps"]) == 18 for g in ref)
    lines = [_moves(ref[k], LENGTHS[k]) for k in range(7)]
    sp = _match(scamd, lines, evaluator, n_slots=3, n_games=7, num_steps=10)
    assert [sp.get_opening(k) for k in range(7)] == lines
    sp.run()
    traces = _finished(sp, 7)
    ties = 0
    for k, (tr, g, L) in enumerate(zip(traces, ref, LENGTHS)):
        assert tr["game_id"] == k
        assert tr["steps"] == g["steps"][L:L + 10], (k, L)
        if len(g["steps"]) <= L + 10:
            assert tr["outcome"] == g["outcome"], (k, L)
        for s in tr["steps"]:
            mx = max(c[1] for c in s[2])
            ties += sum(c[1] == mx for c in s[2]) > 1
    if evaluator == "synth_coarse":
        assert ties > 0   # the random tie-break, keyed by the absolute ply, was exercised
    assert sp.match_tally() == {"a_white": {**ZERO, "unfinished": 7}, "b_white": ZERO}
    sp.close()


# ---------------------------------------------------------------------------------- 2. an outcome carried through a line
@pytest.fixture(scope="module")
def coarse_game_1(orc):
    g0, g1 = (_oracle_game(orc, "synth_coarse", k, 200) for k in (0, 1))
    mate = {"termination": "Checkmate", "winner": "Black"}
    assert len(g0["steps"]) == 110 and g0["outcome"] == mate     # (pins the oracle: the lengths the issue records)
    assert len(g1["steps"]) == 22 and g1["outcome"] == mate
    return g1


@pytest.mark.parametrize("L", [8, 15])
def test_checkmate_is_reached_through_a_line(scamd, coarse_game_1, L):
    sp = _match(scamd, [_moves(coarse_game_1, L)], "synth_coarse", n_slots=1, n_games=1, num_steps=200, first_game_id=1)
    sp.run()
    tr, = _finished(sp, 1)
    assert tr["game_id"] == 1 and len(tr["steps"]) == 22 - L
    assert tr["steps"] == coarse_game_1["steps"][L:]
    assert tr["outcome"] == {"termination": "Checkmate", "winner": "Black"}
    assert sp.match_tally() == {"a_white": {**ZERO, "Black": 1}, "b_white": ZERO}
    sp.close()


# ---------------------------------------------------------------------------------- 3. history, through the network
@pytest.mark.parametrize("line", ["g1f3 g8f6 f3g1 f6g8", "e2e4 a7a6 e4e5 d7d5"], ids=["repetition", "en-passant"])
def test_network_sees_the_lines_history(scamd, line):
    """the planes of the root hold the line's positions and repetition counts, the legal moves its en-passant square: the first
    searched ply equals sc_search from the same move list (same rollout and cpuct, no noise)"""
    line = line.split()
    eng = scamd.Engine(2, 128, seed=1)
    sp = scamd.SelfPlay(eng, n_slots=1, n_games=1, num_steps=2, **HANDLE)
    sp.set_match(eng, eng, colours=0)
    sp.set_openings([line])
    sp.run()
    tr, = _finished(sp, 1)
    _root_q, kids = scamd.search(eng, line, SEARCH["rollout_num"], cpuct=SEARCH["cpuct"], noise=False, seed=5)
    assert [(m, n, q) for m, n, q, _u in tr["steps"][0][2]] == [(m, n, q) for m, n, q, _p in kids]
    assert sum(c[1] for c in kids) == SEARCH["rollout_num"] - 1
    if line[-1] == "d7d5":
        assert "e5d6" in [c[0] for c in kids]
    sp.close()
    eng.close()


# ---------------------------------------------------------------------------------- 4. alternating colours
def test_alternating_colours_share_a_line(scamd):
    from scamd.selfplay import opening_of_game
    lines = [["e2e4"], ["d2d4", "d7d5"], ["g1f3", "g8f6", "c2c4"]]
    sp = _match(scamd, lines, colours=1, n_slots=2, n_games=6, num_steps=8, first_game_id=30)
    sp.run()
    traces = _finished(sp, 6)
    assert sorted(t["game_id"] for t in traces) == list(range(30, 36))
    for k, tr in enumerate(traces):
        assert tr["game_id"] == 30 + k
        assert sp.get_opening(k) == lines[k >> 1] == lines[opening_of_game(k, 3, 1)]
        salts = (SALT_B, SALT_A) if k & 1 else (SALT_A, SALT_B)   # game k's White first
        one = _match(scamd, [lines[k >> 1]], colours=0, salts=salts, n_slots=1, n_games=1, num_steps=8, first_game_id=30 + k)
        one.run()
        want, = _finished(one, 1)
        one.close()
        assert tr == want, k
    tally = sp.match_tally()
    assert sum(tally["a_white"].values()) == 3 and sum(tally["b_white"].values()) == 3
    sp.close()


# ---------------------------------------------------------------------------------- 5. the empty line
def test_empty_line_changes_nothing(scamd, tmp_path):
    cfg = dict(colours=1, n_slots=2, n_games=4, num_steps=6)
    out = []
    for tag, lines in (("none", None), ("empty", [[]])):
        sp = _match(scamd, lines, **cfg)
        sp.run()
        traces = _finished(sp, 4)
        files = []
        for k in range(4):
            path = str(tmp_path / f"{tag}_{k}.json")
            sp.write_trace(k, path)
            files.append(open(path, "rb").read())
        out.append((traces, sp.match_tally(), files))
        assert sp.get_opening(0) == []
        sp.close()
    assert out[0] == out[1]
    assert all(list(json.loads(f).keys()) == ["outcome", "steps"] for f in out[0][2])
    # ... and a line of two plies is written behind the reference's two keys
    sp = _match(scamd, [["e2e4", "c7c5"]], n_slots=1, n_games=1, num_steps=3)
    sp.run()
    _finished(sp, 1)
    path = str(tmp_path / "line.json")
    sp.write_trace(0, path)
    js = json.load(open(path))
    assert list(js.keys()) == ["outcome", "steps", "opening"] and js["opening"] == ["e2e4", "c7c5"] and len(js["steps"]) == 3
    assert open(path).read().endswith('  ],\n  "opening": [\n    "e2e4",\n    "c7c5"\n  ]\n}')
    sp.close()


def test_second_set_openings_replaces_the_first(scamd):
    """a second call replaces the first one's table, moves and bases and draws the slots again: a handle given suite A (a base with
    Black to move: padded records) and then suite B (an odd line, an empty one: not copied) is the handle given suite B alone"""
    suite_a = [("rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq - 0 1", ["c7c5"]), ["d2d4", "d7d5"]]
    suite_b = [["g1f3", "g8f6", "b1c3"], []]
    cfg = dict(n_slots=2, n_games=4, num_steps=6, colours=1)
    x = _match(scamd, suite_a, **cfg)
    assert x.get_opening_fen(0) == suite_a[0][0] and x.get_opening(2) == suite_a[1]
    x.set_openings(suite_b)
    y = _match(scamd, suite_b, **cfg)
    out = []
    for sp in (x, y):
        for k in range(4):
            assert sp.get_opening(k) == suite_b[(k >> 1) % 2] and sp.get_opening_fen(k) is None, k
        sp.run()
        st = sp.stats()
        assert st["error_flags"] == 0
        out.append((st, sp.match_tally(), _finished(sp, 4)))   # (a trace: moves, root q, every child tuple, outcome)
        sp.close()
    assert out[0] == out[1]


# ---------------------------------------------------------------------------------- 6. refusals
FOOLS_MATE = "f2f3 e7e5 g2g4 d8h4".split()
CLAIMABLE = "g1f3 g8f6 f3g1 f6g8 g1f3 g8f6 f3g1".split()   # f6g8 would repeat the start position for the third time


def test_refusals(scamd, orc):
    st = orc.State()
    for m in CLAIMABLE:
        st.push(m)
    assert st.outcome() == {"termination": "ThreefoldRepetition", "winner": None}   # (outcome(claim_draw=True) on the CPU oracle)
    cfg = dict(n_slots=2, n_games=3, num_steps=4)
    sp = _match(scamd, None, **cfg)
    with pytest.raises(scamd.EngineError) as e:
        sp.set_openings([[], ["e2e4", "e7e5", "e1e3"], FOOLS_MATE, CLAIMABLE, ["e2e5"]])
    assert e.value.code == -1 and e.value.status == [0, -3, 1, 1, -1]
    with pytest.raises(scamd.EngineError) as e:
        sp.set_openings([["g1f3", "g8f6", "f3g1", "f6g8"] * 150 + ["g1f3"]])   # 601 plies
    assert e.value.code == -1 and "601" in str(e.value)
    assert sp.get_opening(0) == []
    # after the refused calls the handle plays the games it plays without openings
    sp.run()
    plain = _match(scamd, None, **cfg)
    plain.run()
    assert _finished(sp, 3) == _finished(plain, 3) and sp.match_tally() == plain.match_tally()
    with pytest.raises(scamd.EngineError, match="first enqueue"):
        sp.set_openings([["e2e4"]])
    sp.close()
    plain.close()
    sp = scamd.SelfPlay(None, n_slots=2, n_games=2, evaluator="synth", rollout_num=4, num_steps=4)
    with pytest.raises(scamd.EngineError, match="set_match") as e:
        sp.set_openings([["e2e4"]])
    assert e.value.code == -1
    sp.close()
    # training tensors need the plies from the start: a game with a line is refused, before anything is enqueued
    sp = _match(scamd, [["e2e4"], []], n_slots=2, n_games=2, num_steps=2)
    sp.run()
    _finished(sp, 2)
    games, ply_off = np.zeros(1, np.int32), np.zeros(2, np.uint32)
    args = (1, games.ctypes.data_as(C.c_void_p), 0, 0, None, ply_off.ctypes.data_as(C.c_void_p)) + (None,) * 7
    assert sp.L.sc_selfplay_encode_traces(sp.h, *args) == -1 and "opening line" in sp.L.sc_last_error().decode()
    games[0] = 1   # (the game from the empty line is encoded as ever: the sizing call answers)
    assert sp.L.sc_selfplay_encode_traces(sp.h, *args) == 0 and ply_off[1] == 2
    sp.close()


# ---------------------------------------------------------------------------------- 7. the launcher and the suite generator
def test_play_cli_openings(tmp_path, orc):
    """sc-play --openings --swap: both games of a pair start from the pair's line, and the replay files carry it"""
    suite = tmp_path / "suite.txt"
    suite.write_text("# two lines and the start position\ne2e4 c7c5 g1f3   # odd length\n\nd2d4 d7d5\n")
    lines = [["e2e4", "c7c5", "g1f3"], [], ["d2d4", "d7d5"]]
    common = [PLAY, "--white-device", "cuda", "--black-device", "cuda", "--black-type", "nn", "--rollout=12", "--temperature", "0",
              "--temperature-switch", "0", "--cpuct", "1.5", "--games", "3", "--blocks", "1", "--channels", "128", "--white-seed", "3",
              "--black-seed", "4", "-o", str(tmp_path / "w_{}.json")]
    r = subprocess.run(common + ["--swap", "--swap-output", str(tmp_path / "b_{}.json"), "--concurrency", "4", "--openings", str(suite)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "games 6 slots 4" in r.stdout and "elo.py input: 6/" in r.stdout
    for prefix in "wb":
        for k, line in enumerate(lines, 1):
            js = json.load(open(str(tmp_path / f"{prefix}_{k}.json")))
            assert list(js.keys()) == ["outcome", "steps"] + (["opening"] if line else []), (prefix, k)
            assert js.get("opening", []) == line and 1 <= len(js["steps"]) <= 200
            st = orc.State()
            for mv in line:
                st.push(mv)
            for mv, _q, kids in js["steps"]:
                assert sorted(c[0] for c in kids) == sorted(st.legal_uci()) and sum(c[1] for c in kids) == 11
                st.push(mv)
            assert js["outcome"] == st.outcome()
    # a token that is no move: refused before anything is loaded; a move that is not legal: refused with its line and status
    suite.write_text("e2e4 e7e5\nd2d4 Nf6\n")
    r = subprocess.run(common + ["--openings", str(suite)], capture_output=True, text=True)
    assert r.returncode != 0 and "suite.txt:2" in r.stderr and "Nf6" in r.stderr
    suite.write_text("e2e4 e7e5\n# a comment\nd2d4 d7d5 e1e2\n")
    r = subprocess.run(common + ["--openings", str(suite)], capture_output=True, text=True)
    assert r.returncode != 0 and "suite.txt:3: opening refused, status -3" in r.stderr
    assert not os.path.exists(str(tmp_path / "w_4.json"))


def test_make_openings_counts(scamd, tmp_path):
    import make_openings
    from scamd.selfplay import read_openings
    for plies, count in ((1, 20), (2, 400)):
        lines, dropped = make_openings.generate(plies)
        assert len(lines) == count and dropped == 0 and len({tuple(ln) for ln in lines}) == count
        assert all(len(ln) == plies for ln in lines)
        path = str(tmp_path / f"openings_{plies}.txt")
        make_openings.write(path, lines)
        assert read_openings(path) == lines
        sp = _match(scamd, lines, colours=1, n_slots=2, n_games=4, num_steps=2)   # every line passes the device's check
        assert sp.get_opening(3) == lines[1]
        sp.close()
