"""Positions given as FEN, on the GPU (-m gpu): validated records (sc_positions_from_fen) and, from such a base, the rules and
the encoder, a search, match games and SAN game records.  The yardstick everywhere is the CPU oracle started from the same FEN
(orc.State(fen)); the start position given as a base, or no base, must give what the library gave before it had bases."""
import ctypes as C
import json
import os
from collections import Counter

import numpy as np
import pytest

from helpers import _same_tree
from san_ref import one_hot_steps, san_of, yardstick_moves
from lines import PERFT
from support import TENSORS, _p, _read, alloc_outputs, assert_bit_equal, dev_per_test, run_san, scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu

START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR"
KIWI = "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1"
REF39 = "1k1r4/1r5p/p4n1P/1ppP1P2/PP6/4PP1b/3B4/R1N1K3 b - - 0 39"
EPD = "r1bqkbnr/pppp1ppp/2n5/4p2Q/2B1P3/8/PPPP1PPP/RNB1K1NR w KQkq - bm Qxf7+; id \"scholar\";"
EP_LEGAL = "rnbqkbnr/ppp1p1pp/8/3pPp2/8/8/PPPP1PPP/RNBQKBNR w KQkq f6 0 3"      # e5xf6 is on
EP_UNUSED = "rnbqkbnr/pppp1ppp/8/4p3/4P3/8/PPPP1PPP/RNBQKBNR w KQkq e6 0 2"     # a valid ep square nobody can capture on
EP_BOGUS = START + " w KQkq e6 0 1"                                             # no pawn in front of it: dropped
UNCLEAN = "4k2r/8/8/8/8/8/8/R3K3 w KQkq - 0 1"                                  # rights without their rooks: cleaned to Qk
BARE_KINGS = "4k3/8/8/8/8/8/8/4K3 w - - 0 1"
STALEMATE = "7k/5Q2/6K1/8/8/8/8/8 b - - 0 1"
HALFMOVE_100 = "4k3/8/8/8/8/8/4P3/4K3 w - - 100 80"
HALFMOVE_99 = "4k3/8/8/8/8/8/4P3/4K2R w K - 99 80"
KINGS_ADJACENT = "8/8/8/8/8/8/8/Kk6 w - - 0 1"
NO_BLACK_KING = "8/8/8/8/8/8/8/K7 w - - 0 1"
PAWN_ON_8 = "3P4/8/8/8/8/8/8/K6k w - - 0 1"
NINE_QUEENS = "QQQQQQQQ/Q7/8/8/8/PPPPPPPP/8/K6k w - - 0 1"
TWO_QUEENS_8_PAWNS = "QQ6/8/8/8/8/PPPPPPPP/8/K6k w - - 0 1"
THREE_CHECKERS = "4k3/3P1P2/8/8/4R3/8/8/4K3 b - - 0 1"
SYNTAX = START + " w KQkq e4 0 1"

# one call, refused and playable positions interleaved: (text or None, status)
SUITE = [(list(PERFT)[0], 0), (KINGS_ADJACENT, -3), (list(PERFT)[1], 0), (None, 0), (NO_BLACK_KING, -1), (list(PERFT)[2], 0),
         (PAWN_ON_8, -2), (list(PERFT)[3], 0), (NINE_QUEENS, -4), (list(PERFT)[4], 0), (BARE_KINGS, 1), (list(PERFT)[5], 0),
         (STALEMATE, 1), (REF39, 0), (HALFMOVE_100, 1), (EPD, 0), (EP_BOGUS, 0), (SYNTAX, -104), (EP_LEGAL, 0), (TWO_QUEENS_8_PAWNS, -4),
         (EP_UNUSED, 0), (THREE_CHECKERS, -5), (UNCLEAN, 0), (HALFMOVE_99, 1)]


@pytest.fixture(scope="module")
def fen(scamd):
    import scamd.fen as m
    return m


def _six(text):
    """the six-field form the oracle reads (an EPD record: halfmove 0, fullmove 1)"""
    return START + " w KQkq - 0 1" if text is None else text if text != EPD else " ".join(EPD.split()[:4]) + " 0 1"


def _state(orc, text, moves=()):
    st = orc.State(_six(text))
    for m in moves:
        st.push(m)
    return st


def _first_moves(orc, text, n, first=None):
    """n moves from the position: `first` if given, then the oracle's first legal move each time"""
    st, out = _state(orc, text), []
    for i in range(n):
        if not st.legal_moves():
            break
        m = orc.from_uci(first) if (i == 0 and first) else st.legal_moves()[0]
        st.push(m)
        out.append(orc.uci(m))
    return out


# ---------------------------------------------------------------------------------- 1. canonical records and status
def test_canonical_records_and_status(scamd, fen, orc):
    texts = [t for t, _ in SUITE]
    pos = fen.Positions(texts)
    assert len(pos) == len(SUITE)
    assert pos.status.tolist() == [s for _, s in SUITE]
    assert [scamd.lib().sc_positions_status(pos.h, i) for i in range(len(SUITE))] == [s for _, s in SUITE]
    for i, (t, s) in enumerate(SUITE):
        if s >= 0:
            assert pos.fen(i) == _state(orc, t).fen(), (i, t)
        else:
            buf = C.create_string_buffer(128)
            assert scamd.lib().sc_positions_fen(pos.h, i, buf, 128) < 0 and "refused" in scamd.lib().sc_last_error().decode()
    by = dict(zip(texts, range(len(texts))))
    assert pos.fen(by[EP_BOGUS]).split()[3] == "-" and pos.fen(by[EP_UNUSED]).split()[3] == "-" and pos.fen(by[EP_LEGAL]).split()[3] == "f6"
    assert pos.fen(by[UNCLEAN]).split()[2] == "Qk" and pos.fen(by[None]) == START + " w KQkq - 0 1"
    # n = 1: the same record, whatever stood beside it
    for t in (REF39, EP_LEGAL, HALFMOVE_99):
        one = fen.Positions([t])
        assert one.status.tolist() == [dict(SUITE)[t]] and one.fen(0) == pos.fen(by[t])
        one.close()
    # a short buffer gets a cut text and the whole length
    buf = C.create_string_buffer(b"#" * 16, 16)
    want = pos.fen(by[REF39])
    assert scamd.lib().sc_positions_fen(pos.h, by[REF39], buf, 10) == len(want) and buf.raw[:11] == want[:9].encode() + b"\0#"
    empty = fen.Positions([])
    assert len(empty) == 0 and empty.status.size == 0
    empty.close()
    pos.close()
    # consumers refuse what cannot be played, and a finished game where a search would start
    with pytest.raises(scamd.EngineError, match="cannot be played"):
        scamd.encode_positions([[]], fens=[KINGS_ADJACENT])
    with pytest.raises(scamd.EngineError, match="game is over"):
        scamd.Play(None, fen=STALEMATE, evaluator="synth")


# ---------------------------------------------------------------------------------- 2. rules and encoder from a base
def _check_encoding(scamd, orc, enc, i, st):
    ob, om = st.encode()
    assert np.array_equal(enc["boards"][i], ob) and np.array_equal(enc["meta"][i], om), i
    assert list(enc["legal_moves"][i]) == st.legal_moves(), i
    assert list(enc["legal_idx"][i]) == [orc.move_index(m, st.turn) for m in st.legal_moves()], i
    oc = st.outcome()
    assert scamd.TERMINATION[int(enc["termination"][i])] == (oc["termination"] if oc else None), i
    assert {1: "White", 0: "Black", -1: None}[int(enc["winner"][i])] == (oc["winner"] if oc else None), i
    assert bool(enc["is_check"][i]) == st.is_check() and enc["status"][i] == 0, i


def test_rules_and_encoder_from_a_base(scamd, fen, orc):
    bases = [t for t, s in SUITE if s >= 0 and t is not None]
    cases = [(t, _first_moves(orc, t, n)) for t in bases for n in (0, 1, 9) if n == 0 or _state(orc, t).legal_moves()]
    cases.append((EP_LEGAL, _first_moves(orc, EP_LEGAL, 4, first="e5f6")))     # the en-passant capture itself, and on from there
    cases.append((HALFMOVE_99, ["h1h2"]))                                       # a quiet move: the fiftieth
    plain = [[], ["e2e4", "c7c5", "g1f3"], ["g1f3", "g8f6", "f3g1", "f6g8", "g1f3"]]
    mixed = []
    for k, c in enumerate(cases):                                               # positions without a base among the others
        mixed.append(c)
        if k % 7 == 3:
            mixed.append((None, plain[(k // 7) % 3]))
    mixed.append((None, plain[2]))
    enc = scamd.encode_positions([mv for _, mv in mixed], fens=[t for t, _ in mixed])
    seen = Counter()
    for i, (t, mv) in enumerate(mixed):
        st = _state(orc, t, mv)
        _check_encoding(scamd, orc, enc, i, st)
        seen["black_base"] += t is not None and _six(t).split()[1] == "b"
        seen["older_planes_zero"] += t is not None and len(mv) < 7 and not enc["boards"][i][:, :, 14 * (len(mv) + 1):].any()
        seen["fifty"] += (t, mv) == cases[-1] and scamd.TERMINATION[int(enc["termination"][i])] == "FiftyMoves"
        seen["no_base"] += t is None
    assert seen["black_base"] >= 3 and seen["fifty"] >= 1 and seen["no_base"] >= 3, dict(seen)
    assert seen["older_planes_zero"] == sum(t is not None and len(mv) < 7 for t, mv in mixed)
    assert cases[-2][1][0] == "e5f6" and _state(orc, EP_LEGAL, ["e5f6"]).piece_at(37) == 0      # the pawn on f5 is gone
    # the positions without a base are what encode_positions gives today, bit for bit
    rows = [i for i, (t, _) in enumerate(mixed) if t is None]
    today = scamd.encode_positions([mixed[i][1] for i in rows])
    for k, i in enumerate(rows):
        assert np.array_equal(enc["boards"][i], today["boards"][k]) and np.array_equal(enc["meta"][i], today["meta"][k])
        assert np.array_equal(enc["legal_moves"][i], today["legal_moves"][k]) and np.array_equal(enc["legal_idx"][i], today["legal_idx"][k])
        assert [int(enc[f][i]) for f in ("termination", "winner", "is_check", "status")] == [int(today[f][k]) for f in ("termination", "winner", "is_check", "status")]
    # a shared, validated set works as the list of texts does; an illegal move after a base is reported at its index
    pos = fen.Positions([t for t, _ in mixed[:5]])
    again = scamd.encode_positions([mv for _, mv in mixed[:5]], fens=pos)
    assert np.array_equal(again["boards"], enc["boards"][:5]) and np.array_equal(again["meta"], enc["meta"][:5])
    pos.close()
    bad = scamd.encode_positions([["e2e4"], ["b8c7", "e1e2", "a1a1"]], fens=[REF39, REF39])
    assert bad["status"].tolist() == [-1, -3]


# ---------------------------------------------------------------------------------- 3. search from a base
def _oracle_search(orc, st, sims, depth=0, user=None):
    """sims = [(count, cpuct), ...] on a fresh oracle search of st"""
    srch = orc.Search(st, depth=depth)
    for n, cpuct in sims:
        for _ in range(n):
            srch.sim(cpuct=cpuct, with_noise=False, user=user)
    return srch


@pytest.mark.parametrize("text,n_moves", [(KIWI, 2), (REF39, 0), (REF39, 1)], ids=["kiwipete+2", "black", "black+1"])
def test_search_from_a_base(scamd, orc, text, n_moves):
    moves = _first_moves(orc, text, n_moves)
    pl = scamd.Play(None, fen=text, initial_moves=moves, evaluator="synth")
    st = _state(orc, text, moves)
    assert pl.fen() == st.fen() and pl.base_fen == _state(orc, text).fen()
    pl.mcts(10, cpuct=2.5)
    pl.mcts(15, cpuct=1.25)
    d = _oracle_search(orc, st, [(10, 2.5), (15, 1.25)], depth=n_moves).dump()
    assert _same_tree(pl.sp.tree(0), d)
    _, stack, q, ch = pl.inspect()
    assert stack == list(reversed(moves)) and q == float(d["q"][0]) and [c[0] for c in ch] == st.legal_uci()
    tree = pl.dump_search_tree()
    base_side = "White" if text.split()[1] == "w" else "Black"
    assert tree["step"] == [None, base_side] and tree["depth"] == 0
    cur = tree
    for k in range(n_moves):
        cur = cur["children"][0]
    assert cur["depth"] == n_moves and cur["num_act"] == 25 and cur["step"][1] == ("White" if st.turn else "Black")
    mv = pl.step(0.0)
    best = max(c[1] for c in ch)
    assert mv == next(c[0] for c in ch if c[1] == best)
    st.push(mv)
    assert pl.fen() == st.fen()
    pl.close()


def test_search_from_and_analyse(scamd, fen, orc):
    # sc_search_from: the root children a handle of one's own finds from the same base
    eng = scamd.Engine(1, 128, seed=2)
    moves = _first_moves(orc, REF39, 1)
    root_q, kids = scamd.search(eng, moves, 12, cpuct=1.5, noise=False, seed=5, fen=REF39)
    pl = scamd.Play(eng, fen=REF39, initial_moves=moves, seed=5)
    pl.mcts(12, cpuct=1.5)
    _, _, q, ch = pl.inspect()
    assert [(m, n, w) for m, n, w, _pr in kids] == ch and root_q == q and sum(c[1] for c in kids) == 11
    assert [c[0] for c in kids] == _state(orc, REF39, moves).legal_uci()
    steps, pri, val = pl.inference()
    assert steps == [c[0] for c in kids] and 0.9 < float(pri.sum()) <= 1.0
    b, m = pl.encode()
    ob, om = _state(orc, REF39, moves).encode()
    assert np.array_equal(b, ob) and np.array_equal(m, om)
    pl.close()
    # without a base sc_search_from is sc_search
    assert scamd.search(eng, ["e2e4"], 8, seed=1) == scamd.search(eng, ["e2e4"], 8, seed=1, fen=START + " w KQkq - 0 1")
    eng.close()
    # analyse: three different bases in one handle = three one-slot runs = the oracle's trees
    suite = [KIWI, REF39, list(PERFT)[2]]
    got = fen.analyse(None, suite, 25, cpuct=1.5, evaluator="synth", trees=True)
    assert got["solved"] is None and len(got["results"]) == 3
    for i, t in enumerate(suite):
        one = fen.analyse(None, [t], 25, cpuct=1.5, evaluator="synth", trees=True)["results"][0]
        d = _oracle_search(orc, _state(orc, t), [(25, 1.5)]).dump()
        r = got["results"][i]
        assert _same_tree(r["tree"], d) and _same_tree(one["tree"], d), i
        assert r["children"] == one["children"] and r["move"] == one["move"] and r["fen"] == _state(orc, t).fen()
        assert [c[0] for c in r["children"]] == _state(orc, t).legal_uci()
    best = [r["move"] for r in got["results"]]
    solved = fen.analyse(None, suite, 25, cpuct=1.5, evaluator="synth", best=[best[0], ["a1a1"], {best[2], "h1h8"}])
    assert solved["solved"] == 2


# ---------------------------------------------------------------------------------- 4. match games from bases
SALT_A, SALT_B = 11, 22
W_FEN = "8/2p5/3p4/KP5r/1R3p1k/8/4P1P1/8 w - - 0 1"


def _match(scamd, lines, **kw):
    cfg = dict(seed=5, with_noise=False, outcome_gate=-1, tie_random=True, rollout_num=20, cpuct=1.5, temperature=0.0, temperature_switch=0,
               n_slots=4, n_games=6, num_steps=6)
    sp = scamd.SelfPlay(None, evaluator="synth", **{**cfg, **kw})
    sp.set_match(None, None, SALT_A, SALT_B, colours=1)
    if lines is not None:
        sp.set_openings(lines)
    return sp


def _walk_match(scamd, orc, tmp_path, lines, n_games, **kw):
    """play the handle's games and walk every trace with the oracle from the oracle's State of the game's line"""
    sp = _match(scamd, lines, n_games=n_games, **kw)
    sp.run()
    st = sp.stats()
    assert st["error_flags"] == 0 and st["games_finished"] == n_games and st["games_active"] == 0, st
    tally = {"a_white": Counter(), "b_white": Counter()}
    for k in range(n_games):
        line = lines[(k >> 1) % len(lines)]
        text, moves = line if isinstance(line, tuple) else (None, line)
        assert sp.get_opening(k) == list(moves)
        assert sp.get_opening_fen(k) == (None if text is None else _state(orc, text).fen())
        tr = sp.trace(k)
        assert tr["game_id"] == k and len(tr["steps"]) >= 1
        state = _state(orc, text, moves)
        white_salt, black_salt = (SALT_B, SALT_A) if k & 1 else (SALT_A, SALT_B)      # colours = 1: b is White in the odd games
        for mv, _root_q, kids in tr["steps"]:
            box = C.c_uint64(white_salt if state.turn else black_salt)                 # the player of the side to move
            d = _oracle_search(orc, state, [(20, 1.5)], user=C.cast(C.byref(box), C.c_void_p)).dump()
            nc = int(d["n_child"][0])
            assert [(m, n, q) for m, n, q, _u in kids] == [(orc.uci(d["move"][1 + i]), int(d["n"][1 + i]), float(d["q"][1 + i])) for i in range(nc)], k
            most = max(c[1] for c in kids)
            assert mv in [c[0] for c in kids if c[1] == most], k
            state.push(mv)
        assert tr["outcome"] == state.outcome(), k
        assert len(tr["steps"]) == sp.cfg.num_steps or tr["outcome"] is not None, k
        oc = tr["outcome"]
        tally["b_white" if k & 1 else "a_white"]["unfinished" if oc is None else "draw" if oc["winner"] is None else oc["winner"]] += 1
        path = str(tmp_path / f"game_{k}.json")
        sp.write_trace(k, path)
        js = json.load(open(path))
        if text is None:
            assert list(js.keys()) == ["outcome", "steps", "opening"] and js["opening"] == list(moves)
        else:
            assert list(js.keys()) == ["outcome", "steps", "fen"] + (["opening"] if moves else []), k
            assert js["fen"] == _state(orc, text).fen() and js.get("opening", []) == list(moves)
            assert ('  ],\n  "fen": "%s"' % js["fen"]) in open(path).read()
    got = sp.match_tally()
    assert {w: {r: n for r, n in got[w].items() if n} for w in got} == {w: dict(c) for w, c in tally.items()}
    return sp


def test_match_games_from_bases(scamd, orc, tmp_path):
    """6 games on 4 recycled slots, colours = 1: a White-to-move FEN with no moves, a Black-to-move FEN with one move, a plain line"""
    lines = [(W_FEN, []), (REF39, _first_moves(orc, REF39, 1)), ["e2e4", "c7c5", "g1f3"]]
    sp = _walk_match(scamd, orc, tmp_path, lines, 6)
    # training tensors from the trace ring: a game from a base is refused like every game with a line
    games, ply_off = np.zeros(1, np.int32), np.zeros(2, np.uint32)
    args = (1, games.ctypes.data_as(C.c_void_p), 0, 0, None, ply_off.ctypes.data_as(C.c_void_p)) + (None,) * 7
    assert sp.L.sc_selfplay_encode_traces(sp.h, *args) == -1 and "opening line" in sp.L.sc_last_error().decode()
    sp.close()


def test_match_game_whose_first_ply_is_blacks(scamd, orc, tmp_path):
    """a Black-to-move base with no moves (and with two): the first searched ply belongs to Black's player, in both colour assignments"""
    sp = _walk_match(scamd, orc, tmp_path, [(REF39, []), (REF39, _first_moves(orc, REF39, 2))], 4, n_slots=2, num_steps=3)
    sp.close()
    # before the first step: the game whose Black is player a has started, at the base; its root is the base's record
    sp = _match(scamd, [(REF39, [])], n_slots=2, n_games=2, num_steps=3)
    active = [g for g in range(2) if sp.slot(g)["status"] == 1]
    assert len(active) == 1 and sp.slot(active[0])["game_id"] == 1 and sp.fen(active[0]) == _state(orc, REF39).fen()
    with pytest.raises(scamd.EngineError, match="holds no game"):
        sp.fen(1 - active[0])
    sp.close()


def test_match_lines_refuse_bad_bases(scamd, orc):
    sp = _match(scamd, None, n_slots=2, n_games=2, num_steps=3)
    for bad, status in (([(W_FEN, []), (STALEMATE, [])], [0, 1]), ([(KINGS_ADJACENT, []), ["e2e4"]], [-3, 0]),
                        ([(REF39, ["e1e2"])], [-1]), ([(HALFMOVE_99, ["h1h2"])], [1])):
        with pytest.raises(scamd.EngineError) as e:
            sp.set_openings(bad)
        assert e.value.code == -1 and e.value.status == status, bad
        assert sp.get_opening(0) == [] and sp.get_opening_fen(0) is None
    # the handle is as before: it plays the games a handle without lines plays
    sp.run()
    plain = _match(scamd, None, n_slots=2, n_games=2, num_steps=3)
    plain.run()
    assert [sp.trace(k) for k in range(2)] == [plain.trace(k) for k in range(2)]
    sp.close()
    plain.close()


# ---------------------------------------------------------------------------------- 5. SAN and training tensors from a base
def _walk(orc, text, n, seed):
    """a game of n plies from the position, moves drawn from the oracle's legal moves: (moves, SAN movetext, one-hot steps)"""
    rng = np.random.default_rng(seed)
    st = _state(orc, text)
    moves, words, steps, seen = [], [], [], Counter()
    for _ in range(n):
        legal = st.legal_moves()
        if not legal:
            break
        m = legal[int(rng.integers(len(legal)))]
        words.append(san_of(st, m, "min", seen))
        steps.append((m, [(x, 1 if x == m else 0) for x in legal]))
        st.push(m)
        moves.append(m)
    return moves, " ".join(words), steps


def _run_from(scamd, dev, call, n, P, head, mirror, layout, with_moves):
    o = alloc_outputs(dev, P, n, layout, skip=() if with_moves else ("moves",))
    tail = [o[k] for k in TENSORS] + ([o["moves"]] if with_moves else []) + [o["status"]]
    rc = call(None, 0, n, *head, int(mirror), layout, dev.stream, *tail)
    assert rc == 0, scamd.lib().sc_last_error().decode()
    dev.sync()
    return _read(dev, o, P, n, layout)


@pytest.mark.parametrize("mirror,layout", [(False, 0), (True, 1)])
def test_san_and_training_tensors_from_a_base(scamd, fen, orc, dev, mirror, layout):
    import scamd.san as san
    golden, _w = san.read_games_csv(os.path.join(os.path.dirname(__file__), "golden", "ref_sample_games.csv"), limit=1)
    g_moves = yardstick_moves(orc, golden[0])
    walks = [_walk(orc, KIWI, 12, 1), _walk(orc, REF39, 11, 2)]
    assert all(len(w[0]) >= 8 for w in walks)
    texts = [walks[0][1], golden[0], walks[1][1]]                      # the start-position game between the two
    steps = [walks[0][2], one_hot_steps(orc, g_moves), walks[1][2]]
    want = [walks[0][0], g_moves, walks[1][0]]
    pos = fen.Positions([KIWI, REF39])
    base_idx = np.asarray([0, -1, 1], np.int32)
    tokens, off = san.pack_tokens(texts)
    P = int(off[-1])
    L = scamd.lib()
    r = _run_from(scamd, dev, L.sc_encode_san_device_from, 3, P, (pos.h, _p(base_idx), _p(tokens), _p(off)), mirror, layout, True)
    assert r["status"].tolist() == [0, 0, 0]
    assert np.array_equal(r["moves"], np.asarray([m for g in want for m in g], np.uint16))
    mv, moff, cm, cn, coff = scamd.pack_steps(steps)
    ref = _run_from(scamd, dev, L.sc_encode_steps_device_from, 3, P, (pos.h, _p(base_idx), _p(mv), _p(moff), _p(cm), _p(cn), _p(coff)),
                    mirror, layout, False)
    assert ref["status"].tolist() == [0, 0, 0]
    assert_bit_equal(r, ref, keys=TENSORS)
    # the game from the start position: the rows sc_encode_san_device gives for it alone, today's entry point
    alone = run_san(scamd, san, dev, [golden[0]], mirror, layout)
    assert_bit_equal({k: v[off[1]:off[2]] for k, v in r.items() if k in TENSORS + ("moves",)}, alone)
    if layout == 0 and not mirror:
        # ... and the rows of the games from bases are the oracle's positions: planes and meta of every ply
        for g, text in ((0, KIWI), (2, REF39)):
            st = _state(orc, text)
            for p, m in enumerate(want[g]):
                ob, om = st.encode()
                assert np.array_equal(r["boards"][off[g] + p], ob) and np.array_equal(r["meta"][off[g] + p], om), (g, p)
                assert r["n_legal"][off[g] + p] == len(st.legal_moves())
                st.push(m)
        # a SAN move that is not legal from the base is reported at its ply; a base that cannot be played is refused
        bad = san.pack_tokens(["Kc7 Ke2 Qd4"])
        b = _run_from(scamd, dev, L.sc_encode_san_device_from, 1, 3, (pos.h, _p(np.asarray([1], np.int32)), _p(bad[0]), _p(bad[1])), 0, 0, True)
        assert b["status"].tolist() == [-3]
        refused = fen.Positions([KINGS_ADJACENT])
        st_buf = dev.alloc(4)
        rc = L.sc_encode_san_device_from(None, 0, 1, refused.h, _p(np.zeros(1, np.int32)), _p(bad[0]), _p(bad[1]), 0, 0, dev.stream,
                                         None, None, None, None, None, None, None, st_buf)
        assert rc == -1 and "cannot be played" in L.sc_last_error().decode()
        refused.close()
    pos.close()
