"""Match play against an outside opponent (-m gpu): sc_selfplay_set_external / _external_search / _external_wait / _push_moves.
A handle whose opponent replays one side of the oracle's match games (src/play.rs:241-343 restated) must give those games: the
engine's plies bit for bit, the opponent's plies as the reference records an outside player's ply (every legal move a child, one
visit on the move played, values 0), the same outcome and length -- whichever slot a game lands in and whoever ends it."""
import importlib

import numpy as np
import pytest

import external_ref as xr
import lines
from helpers import EDGE_CATEGORIES, load_edge_lines
from support import FILL, _p, scamd_gpu, untouched  # noqa: F401

pytestmark = pytest.mark.gpu

SALT_A, SALT_B = 0x1111, 0x2222   # the engine, the opponent
SEARCH = dict(rollout_num=16, cpuct=1.5, temperature=0.0, temperature_switch=2)
HANDLE = dict(evaluator="synth", seed=21, first_game_id=40, with_noise=False, outcome_gate=-1, tie_random=True, **SEARCH)
N_GAMES = 14
ST_ACTIVE, ST_PENDING = 1, 3
KEYS = ("White", "Black", "draw", "unfinished")


@pytest.fixture(scope="module")
def ext(scamd):
    return importlib.import_module("scamd.external")


def _oracle_games(orc, colours, n, num_steps=200):
    games = {}
    for k in range(n):
        w, b = (SALT_A, SALT_B) if xr.engine_white(colours, k) else (SALT_B, SALT_A)
        games[k] = orc.match_game(user_white=w, user_black=b, seed=21, game_id=40 + k, num_steps=num_steps, **SEARCH)
    return games


def _ended_by_engine(game, colours, k):
    return xr.engine_moves_ply(colours, k, len(game["steps"]) - 1)


@pytest.fixture(scope="module")
def oracle_games(orc):
    """the 14 reference games with alternating colours, and what makes them a test: both sides end games, by mate, by a draw
    claim and by the ply cap"""
    games = _oracle_games(orc, 1, N_GAMES)
    term = lambda k: games[k]["outcome"] and games[k]["outcome"]["termination"]
    n = {k: len(g["steps"]) for k, g in games.items()}
    for k in (10, 12):
        assert term(k) == "Checkmate" and not _ended_by_engine(games[k], 1, k), k      # a pushed mate
    for k in (1, 2, 6):
        assert term(k) == "Checkmate" and _ended_by_engine(games[k], 1, k), k          # the engine's mate
    assert term(8) == "ThreefoldRepetition" and _ended_by_engine(games[8], 1, 8)
    for k in (0, 4):
        assert n[k] == 200 and games[k]["outcome"] is None and not _ended_by_engine(games[k], 1, k), k   # the cap on a pushed ply
    for k in (3, 5):
        assert n[k] == 200 and games[k]["outcome"] is None and _ended_by_engine(games[k], 1, k), k       # ... on a searched ply
    assert min(n.values()) >= 48 and max(n.values()) == 200 and any(v & 1 for v in n.values()), n
    return games


def _run(scamd, ext, orc, games, colours, n_games, n_slots=4, on_round=None, **cfg):
    sp = scamd.SelfPlay(None, n_slots=n_slots, n_games=n_games, num_steps=200, **{**HANDLE, **cfg})
    sp.set_external(None, SALT_A, colours)
    ext.run_external(sp, ext.ScriptedOpponent(xr.script_table(orc, {k: g["steps"] for k, g in games.items()}, colours)), on_round)
    return sp


def _assert_games(traces, games, colours):
    for k, ref in games.items():
        tr = traces[k]
        assert tr is not None and tr["game_id"] == 40 + k, k
        assert len(tr["steps"]) == len(ref["steps"]), k
        assert tr["steps"] == xr.expected_steps(ref["steps"], colours, k), k
        assert tr["outcome"] == ref["outcome"], k


@pytest.fixture(scope="module")
def external(scamd, ext, orc, oracle_games):
    sp = _run(scamd, ext, orc, oracle_games, 1, N_GAMES)
    out = dict(stats=sp.stats(), tally=sp.match_tally(), traces=[sp.trace(k) for k in range(N_GAMES)])
    sp.close()
    return out


def test_games_equal_the_oracles_match_games(external, oracle_games):
    _assert_games(external["traces"], oracle_games, 1)


@pytest.mark.parametrize("colours", [0, 2])
def test_one_colour_for_every_game(scamd, ext, orc, colours):
    games = _oracle_games(orc, colours, 4)
    sp = _run(scamd, ext, orc, games, colours, 4)
    _assert_games([sp.trace(k) for k in range(4)], games, colours)
    tally = sp.match_tally()
    assert sum(tally["b_white" if colours == 0 else "a_white"].values()) == 0
    assert sum(tally["a_white" if colours == 0 else "b_white"].values()) == 4
    sp.close()


def _result(trace):
    oc = trace["outcome"]
    return "unfinished" if oc is None else "draw" if oc["winner"] is None else oc["winner"]


def test_tally_counts_the_games_by_the_engines_colour(external):
    want = {k: dict.fromkeys(KEYS, 0) for k in ("a_white", "b_white")}
    for k, t in enumerate(external["traces"]):
        want["a_white" if xr.engine_white(1, k) else "b_white"][_result(t)] += 1
    assert external["tally"] == want
    assert sum(sum(v.values()) for v in want.values()) == N_GAMES
    st = external["stats"]
    assert st["games_finished"] == N_GAMES and st["games_active"] == 0 and st["error_flags"] == 0


def test_trace_ring_drained_between_rounds(scamd, ext, orc, oracle_games, external):
    traces, seen = {}, []

    def drain(sp):
        seen.extend(sp.slot(i)["status"] for i in range(4))
        for g in sp.poll():
            traces[g] = sp.trace(g)

    sp = _run(scamd, ext, orc, oracle_games, 1, N_GAMES, on_round=drain, trace_capacity=8, trace_hold=True)
    drain(sp)
    st = sp.stats()
    assert st["games_finished"] == N_GAMES and st["games_active"] == 0 and st["error_flags"] == 0
    assert sp.match_tally() == external["tally"]
    sp.close()
    assert ST_PENDING not in seen and ST_ACTIVE in seen
    assert sorted(traces) == list(range(N_GAMES))
    _assert_games(traces, oracle_games, 1)


# ------------------------------------------------------------------ pushed moves of every kind, on an ordinary handle
def _edge_lines():
    """one line per category of the corpus (the first), grouped by length: the lines of a group share a handle"""
    by_cat = {}
    for ln in load_edge_lines():
        by_cat.setdefault(ln["category"], ln)
    assert set(by_cat) == set(EDGE_CATEGORIES)
    groups = {}
    for ln in by_cat.values():
        groups.setdefault(len(ln["uci"]), []).append(ln)
    return groups


def test_pushed_lines_of_the_edge_corpus(scamd, orc):
    """Every line is pushed move by move, all lines of a length in one call per ply; then the position is the oracle's, and after
    one searched ply (which ends the games: num_steps = length + 1, or no legal move) the finished traces hold the lines with the
    oracle's legal moves as children"""
    n_lines = 0
    for length, group in sorted(_edge_lines().items()):
        n = len(group)
        sp = scamd.SelfPlay(None, n_slots=n, n_games=n, evaluator="synth", rollout_num=4, num_steps=length + 1, with_noise=False,
                            outcome_gate=1 << 30, seed=5)
        for i in range(length):
            status = sp.push_moves(list(range(n)), [ln["uci"][i] for ln in group])
            assert status == [0] * n, (length, i, status)
        states = [lines.pushed(orc, ln["uci"]) for ln in group]
        for s, (ln, st) in enumerate(zip(group, states)):
            assert sp.fen(s) == st.fen(), ln["name"]
            assert sp.slot(s)["ply"] == length and sp.slot(s)["sim"] == 0
        sp.run()
        assert sp.stats()["error_flags"] == 0 and sp.stats()["games_active"] == 0
        for s, (ln, st) in enumerate(zip(group, states)):
            tr = sp.trace(s)
            assert tr is not None and len(tr["steps"]) == length + (1 if st.legal_moves() else 0), ln["name"]
            assert [x[0] for x in tr["steps"][:length]] == ln["uci"], ln["name"]
            assert tr["steps"][:length] == [xr.pushed_step(x) for x in tr["steps"][:length]], ln["name"]
            xr.legal_replay(orc, tr["steps"])
        sp.close()
        n_lines += n
    assert n_lines == len(EDGE_CATEGORIES)


def test_pushed_mate_and_pushed_threefold_end_the_game(scamd, orc):
    shuffle = ["g1f3", "g8f6", "f3g1", "f6g8"] * 3
    st = orc.State()
    n_rep = 0
    while st.outcome() is None:   # the oracle's ply and termination of the claimed draw
        st.push(shuffle[n_rep])
        n_rep += 1
    assert 4 < n_rep <= len(shuffle) and st.outcome()["termination"] == "ThreefoldRepetition"
    sp = scamd.SelfPlay(None, n_slots=2, n_games=2, evaluator="synth", rollout_num=4, num_steps=50, with_noise=False, outcome_gate=-1)
    for i in range(4):
        status = sp.push_moves([0, 1], [lines.MATED[i], shuffle[i]])
        assert status == [1 if i == 3 else 0, 0], (i, status)
    for i in range(4, n_rep):
        assert sp.push_moves([1], [shuffle[i]]) == [1 if i == n_rep - 1 else 0], i
    mated, drawn = sp.trace(0), sp.trace(1)
    assert mated["outcome"] == {"termination": "Checkmate", "winner": "Black"} and [s[0] for s in mated["steps"]] == lines.MATED
    assert drawn["outcome"] == st.outcome() and [s[0] for s in drawn["steps"]] == shuffle[:n_rep]
    assert sp.push_moves([0], ["e2e4"]) == [-2]   # the slot holds no game any more
    assert sp.stats()["games_finished"] == 2
    sp.close()


# ------------------------------------------------------------------ refusals
def _snapshot(sp, slot, game):
    s = sp.slot(slot)
    s["path"] = s["path"].tolist()
    tree = {k: v.tobytes() for k, v in sp.tree(slot).items()}
    return s, sp.fen(slot), tree, sp.trace(game)


def test_refused_moves_change_nothing(scamd):
    sp = scamd.SelfPlay(None, n_slots=2, n_games=2, evaluator="synth", rollout_num=8, num_steps=20, with_noise=False, outcome_gate=-1)
    assert sp.push_moves([], []) == []
    before = [_snapshot(sp, s, s) for s in range(2)]
    assert sp.push_moves([0, 1], ["e2e5", "e7e5"]) == [-1, -1]   # not a move of the piece; not the side to move
    assert sp.push_moves([1], ["e7e8q"]) == [-1]
    assert [_snapshot(sp, s, s) for s in range(2)] == before
    with pytest.raises(scamd.EngineError, match="twice"):
        sp.push_moves([1, 1], ["e2e4", "d2d4"])
    with pytest.raises(scamd.EngineError, match="slot 2"):
        sp.push_moves([2], ["e2e4"])
    assert [_snapshot(sp, s, s) for s in range(2)] == before
    sp.enqueue(3)   # in mid-search
    before = [_snapshot(sp, s, s) for s in range(2)]
    assert before[0][0]["sim"] == 3
    assert sp.push_moves([0, 1], ["e2e4", "e2e4"]) == [-2, -2]
    assert [_snapshot(sp, s, s) for s in range(2)] == before
    sp.close()
    # an external handle: the engine is to move in every slot of a fresh handle on which it is White
    sp = scamd.SelfPlay(None, n_slots=2, n_games=4, evaluator="synth", rollout_num=8, num_steps=20, with_noise=False, outcome_gate=-1)
    sp.set_external(None, SALT_A, 0)
    assert sp.external_wait() == []
    before = [_snapshot(sp, s, s) for s in range(2)]
    assert sp.push_moves([0, 1], ["e2e4", "d2d4"]) == [-2, -2]
    assert [_snapshot(sp, s, s) for s in range(2)] == before
    sp.close()


def test_a_listed_twice_slot_returns_minus_one(scamd):
    sp = scamd.SelfPlay(None, n_slots=2, n_games=2, evaluator="synth", rollout_num=8, num_steps=20)
    slots, moves, status = np.array([0, 0], np.int32), np.array([scamd.uci_move("e2e4")] * 2, np.uint16), np.full(2, 7, np.int32)
    assert scamd.lib().sc_selfplay_push_moves(sp.h, 2, _p(slots), _p(moves), _p(status)) == -1
    assert status.tolist() == [7, 7] and sp.slot(0)["ply"] == 0
    sp.close()


def test_external_handle_refusals(scamd):
    mk = lambda **kw: scamd.SelfPlay(None, **{**dict(n_slots=2, n_games=4, evaluator="synth", rollout_num=4, num_steps=8, outcome_gate=-1), **kw})
    sp = mk()
    sp.set_external(None, SALT_A, 2)
    for call in (lambda: sp.enqueue(1), lambda: sp.run(), lambda: sp.set_match(None, None, 1, 2), lambda: sp.set_players(None, None, 1, 2),
                 lambda: sp.set_openings([["e2e4"]]), lambda: scamd.enqueue_interleaved([sp], 1), lambda: sp.set_external(None, 1, 0)):
        with pytest.raises(scamd.EngineError):
            call()
    with pytest.raises(scamd.EngineError, match="wait for the opponent"):   # the opponent is White in both slots
        sp.external_search()
    assert [r["slot"] for r in sp.external_wait()] == [0, 1]
    sp.close()
    for kw, why in ((dict(outcome_gate=100), "outcome_gate"), (dict(rollout_num=300, rollout_factor=2.0), "fixed rollout")):
        sp = mk(**kw)
        with pytest.raises(scamd.EngineError, match=why):
            sp.set_external(None, SALT_A, 0)
        sp.close()
    sp = mk()
    with pytest.raises(scamd.EngineError, match="colours"):
        sp.set_external(None, SALT_A, 3)
    with pytest.raises(scamd.EngineError, match="set_external"):   # a plain handle has no opponent to wait for
        sp.external_search()
    with pytest.raises(scamd.EngineError, match="set_external"):
        sp.external_wait()
    sp.enqueue(1)
    with pytest.raises(scamd.EngineError, match="first enqueue"):
        sp.set_external(None, SALT_A, 0)
    sp.close()


# ------------------------------------------------------------------ external_wait
def test_external_wait_lists_the_waiting_slots_in_order(scamd, orc):
    sp = scamd.SelfPlay(None, n_slots=4, n_games=N_GAMES, num_steps=200, **HANDLE)
    sp.set_external(None, SALT_A, 0)
    assert sp.external_wait() == []
    sp.external_search()
    reqs = sp.external_wait(moves=True)
    assert [r["slot"] for r in reqs] == [0, 1, 2, 3] and [r["game"] for r in reqs] == [0, 1, 2, 3] and [r["ply"] for r in reqs] == [1] * 4
    games = _oracle_games(orc, 0, 4, num_steps=2)
    for r in reqs:
        assert r["fen"] == sp.fen(r["slot"])
        assert r["moves"] == [games[r["game"]]["steps"][0][0]]
    # a buffer one byte (one entry, one move) too small: -1, and nothing is written
    L, G = scamd.lib(), 4
    nbytes = sum(len(r["fen"]) + 1 for r in reqs)

    def call(cap, fens_cap, moves_cap):
        bufs = [np.full(G, FILL * 0x01010101, np.uint32).view(np.int32) for _ in range(3)]
        fens, foff = np.full(nbytes, FILL, np.uint8), np.full(G + 1, FILL * 0x01010101, np.uint32)
        mv, moff = np.full(G, FILL * 0x0101, np.uint16), np.full(G + 1, FILL * 0x01010101, np.uint32)
        rc = L.sc_selfplay_external_wait(sp.h, cap, *[_p(b) for b in bufs], _p(fens), fens_cap, _p(foff), _p(mv), moves_cap, _p(moff))
        return rc, bufs + [fens, foff, mv, moff]

    for args in ((3, nbytes, 4), (4, nbytes - 1, 4), (4, nbytes, 3)):
        rc, out = call(*args)
        assert rc == -1 and all(untouched(a) for a in out), args
    rc, out = call(4, nbytes, 4)
    assert rc == 4 and out[0].tolist() == [0, 1, 2, 3] and out[4].tolist() == [0] + list(np.cumsum([len(r["fen"]) + 1 for r in reqs]))
    assert out[3].tobytes() == b"".join(r["fen"].encode() + b"\0" for r in reqs) and out[6].tolist() == [0, 1, 2, 3, 4]
    assert L.sc_selfplay_external_wait(sp.h, 0, None, None, None, None, 0, None, None, 0, None) == 4   # the count alone
    sp.close()


# ------------------------------------------------------------------ the network path
def test_network_plies_bit_identical_to_the_lockstep_form(scamd, ext, orc):
    a, b = scamd.Engine(2, 128, seed=1), scamd.Engine(1, 128, seed=2)
    cfg = dict(rollout_num=8, num_steps=24, seed=3, first_game_id=0, cpuct=1.5, temperature=0.0, temperature_switch=0, with_noise=False,
               outcome_gate=-1, tie_random=True)
    for n, launches in ((4, 2), (64, 1)):
        sp = scamd.SelfPlay(a, n_slots=n, n_games=n, **cfg)
        sp.set_players(a, b)
        sp.run()
        assert sp.stats()["error_flags"] == 0
        lock = {k: sp.trace(k) for k in range(n)}
        sp.close()
        assert all(t is not None and len(t["steps"]) >= 1 for t in lock.values())
        sp = scamd.SelfPlay(a, n_slots=n, n_games=n, **cfg)
        sp.set_external(a, 0, 0)
        assert sp.launches_per_step() == launches
        ext.run_external(sp, ext.ScriptedOpponent(xr.script_table(orc, {k: t["steps"] for k, t in lock.items()}, 0)))
        st = sp.stats()
        assert st["error_flags"] == 0 and st["games_finished"] == n and st["games_active"] == 0
        for k in range(n):
            tr = sp.trace(k)
            assert tr["steps"] == xr.expected_steps(lock[k]["steps"], 0, k), (n, k)   # the engine's moves, visit counts and every float
            assert tr["outcome"] == lock[k]["outcome"], (n, k)
        sp.close()
    a.close()
    b.close()


# ------------------------------------------------------------------ a random opponent, through play_external
def test_random_opponent_games_replay_legally(scamd, ext, orc):
    r = ext.play_external(None, ext.RandomOpponent(seed=5), n_games=8, concurrency=4, rollout=8, num_steps=60, seed=2, colours=1,
                          evaluator="synth", salt=SALT_A)
    assert set(r) == {"traces", "tally", "elo", "total", "wins", "losses"} and r["total"] == 8 and len(r["traces"]) == 8
    want = {k: dict.fromkeys(KEYS, 0) for k in ("a_white", "b_white")}
    for k, t in enumerate(r["traces"]):
        assert t is not None and 1 <= len(t["steps"]) <= 60, k
        st = xr.legal_replay(orc, t["steps"])
        assert t["outcome"] == st.outcome() and (t["outcome"] is not None or len(t["steps"]) == 60), k
        for i, s in enumerate(t["steps"]):
            if not xr.engine_moves_ply(1, k, i):
                assert s == xr.pushed_step(s), (k, i)
        want["a_white" if xr.engine_white(1, k) else "b_white"][_result(t)] += 1
    assert r["tally"] == want and sum(sum(v.values()) for v in want.values()) == 8
    assert r["wins"] == want["a_white"]["White"] + want["b_white"]["Black"]
    assert r["elo"] == scamd.elo(8, r["wins"], r["losses"])
