"""Games written as SAN and PGN on the GPU (-m gpu): sc_moves_to_san_device, one wavefront per ply, and what stands on it
(sc_selfplay_write_pgn, sc-play --pgn, tools/trace_to_pgn.py, scamd.san.moves_to_san).
Two yardsticks, neither of which calls the device: the words of the reference's own 60 games (tests/golden/ref_sample_games.csv,
read to moves by helpers.san_to_move over the CPU oracle), and san_ref.py's renderer, python-chess's Board.san() over orc.State.
All comparisons are exact text or exact integers.  Device buffers come from hipMalloc on the HIP runtime libsc_engine.so uses,
pre-filled with 0x5a, with guard words behind tokens[P) and status[n), on a non-default stream; this file does not import torch
-- the torch-facing calls run in child processes."""
import json
import os
import re
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

import helpers as H
from san_ref import cpu_game
from support import GOLD, ROOT, _p, dev_per_test, run_torch_child, scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu
PLAY = os.path.join(ROOT, "smart-chess-rust_amd", "lib", "sc-play")
GUARD = 4   # words behind each output
FILL64, FILL32 = 0x5a5a5a5a5a5a5a5a, 0x5a5a5a5a


@pytest.fixture(scope="module")
def san(scamd):
    import scamd.san as m
    return m


def census(words):
    bare = [w.rstrip("+#") for w in words]
    return {"#": sum(w.endswith("#") for w in words), "+": sum(w.endswith("+") for w in words), "O-O": bare.count("O-O"),
            "O-O-O": bare.count("O-O-O"), "file_dis": sum(bool(re.match(r"[NBRQK][a-h]x?[a-h][1-8]$", w)) for w in bare),
            "rank_dis": sum(bool(re.match(r"[NBRQK][1-8]x?[a-h][1-8]$", w)) for w in bare),
            "file_and_rank": sum(bool(re.match(r"[NBRQK][a-h][1-8]x?[a-h][1-8]$", w)) for w in bare), "len7": sum(len(w) == 7 for w in words)}


# ------------------------------------------------------------------ the device call
def pack(games):
    off = np.zeros(len(games) + 1, np.uint32)
    off[1:] = np.cumsum([len(g) for g in games])
    return np.asarray([m for g in games for m in g] or [0], np.uint16), off


def run_write(scamd, san, dev, games, bases=None, base_idx=None):
    """sc_moves_to_san_device[_from] on the test's stream -> (words per game up to the first 0 token, status [n], tokens [P]);
    the guard words behind both outputs must be untouched"""
    L = scamd.lib()
    flat, off = pack(games)
    n, P = len(games), int(off[-1])
    d_tok, d_st = dev.alloc((P + GUARD) * 8), dev.alloc((n + GUARD) * 4)
    if bases is None:
        rc = L.sc_moves_to_san_device(0, n, _p(flat), _p(off), dev.stream, d_tok, d_st)
    else:
        rc = L.sc_moves_to_san_device_from(0, n, bases.h, _p(np.asarray(base_idx, np.int32)), _p(flat), _p(off), dev.stream, d_tok, d_st)
    assert rc == 0, L.sc_last_error().decode()
    dev.sync()
    tok, st = dev.read(d_tok, (P + GUARD,), np.uint64), dev.read(d_st, (n + GUARD,), np.uint32)
    assert (tok[P:] == FILL64).all() and (st[n:] == FILL32).all(), "guard words overwritten"
    tok, st = tok[:P], st[:n].view(np.int32)
    assert not (st == np.int32(FILL32)).any(), "status not filled"
    words = []
    for g in range(n):
        row = [san.token_text(t) for t in tok[off[g]:off[g + 1]]]
        words.append(row[:row.index("")] if "" in row else row)
    return words, st.tolist(), tok


@pytest.fixture(scope="module")
def golden(orc, san):
    """the reference's 60 games: the CSV's words, and their moves by the existing yardstick (helpers.san_to_move over the oracle)"""
    texts, _ = san.read_games_csv(os.path.join(GOLD, "ref_sample_games.csv"))
    words = [t.split() for t in texts]
    moves = []
    for g in words:
        st = orc.State()
        mv = []
        for w in g:
            m, _, _ = H.san_to_move(st, w, orc)
            st.push(m)
            mv.append(m)
        moves.append(mv)
    return dict(words=words, moves=moves)


@pytest.fixture(scope="module")
def edge(orc):
    """the edge-line corpus: moves, and the CPU renderer's words with its counts"""
    seen = Counter()
    moves = [[orc.from_uci(u) for u in ln["uci"]] for ln in H.load_edge_lines()]
    return dict(moves=moves, words=[cpu_game(orc, g, seen=seen) for g in moves], seen=seen)


# ------------------------------------------------------------------ 1. the reference's games
def test_reference_games_word_for_word(scamd, san, orc, dev, golden):
    words, status, _ = run_write(scamd, san, dev, golden["moves"])
    assert status == [0] * 60
    assert words == golden["words"]
    flat = [w for g in words for w in g]
    assert len(flat) == 3539 and max(len(g) for g in words) == 163
    c = census(flat)
    assert (c["#"], c["+"], c["O-O"], c["O-O-O"], c["file_dis"], c["rank_dis"]) == (11, 326, 71, 7, 79, 8), c
    seen = Counter()
    assert [cpu_game(orc, g, seen=seen) for g in golden["moves"]] == golden["words"]   # the CPU renderer agrees with the file too
    assert seen["ep"] == 1 and seen["pinned_rival"] == 1, dict(seen)


# ------------------------------------------------------------------ 2. the edge corpus
def test_edge_corpus_against_the_cpu_renderer(scamd, san, orc, dev, edge):
    moves, want, seen = edge["moves"], edge["words"], edge["seen"]
    assert len(moves) == 90 and sum(len(g) for g in moves) == 4408 and max(len(g) for g in moves) == 198
    c = census([w for g in want for w in g])
    assert (seen["ep"], seen["promo_capture_check"], seen["underpromo"]) == (34, 7, 22), dict(seen)
    assert (c["O-O-O"], c["O-O"], c["#"], c["+"], c["len7"]) == (8, 1, 4, 503, 9), c
    assert c["file_and_rank"] >= 1 and seen["file_and_rank"] == c["file_and_rank"]
    words, status, tok = run_write(scamd, san, dev, moves)
    assert status == [0] * 90
    assert words == want
    # ... and the device's own text goes back through the device parser: moves + status only
    L = scamd.lib()
    tokens, off = san.pack_tokens([san.movetext(g) for g in words])
    P = int(off[-1])
    d_mv, d_st = dev.alloc(P * 2), dev.alloc(90 * 4)
    rc = L.sc_encode_san_device(None, 0, 90, _p(tokens), _p(off), 0, 0, dev.stream, None, None, None, None, None, None, d_mv, d_st)
    assert rc == 0, L.sc_last_error().decode()
    dev.sync()
    assert dev.read(d_st, (90,), np.int32).tolist() == [0] * 90
    assert dev.read(d_mv, (P,), np.uint16).tolist() == [m for g in moves for m in g]


# ------------------------------------------------------------------ 3. bases
THREE_QUEENS = "8/k7/8/8/4Q2Q/8/8/K6Q w - - 0 1"
IN_CHECK = "8/8/8/k7/4Q2Q/8/8/K3r2Q w - - 0 1"
STALEMATE = "7k/8/6K1/5Q2/8/8/8/8 w - - 0 1"
BLACK_12 = "r1bqkbnr/pppp1ppp/2n5/4p3/4P3/5N2/PPPP1PPP/RNBQKB1R b KQkq - 2 12"
BASED = [(THREE_QUEENS, "h4e1", "Qh4e1"), (IN_CHECK, "h4e1", "Qh4xe1+"), (IN_CHECK, "e4e1", "Qexe1+"), (IN_CHECK, "h1e1", "Q1xe1+"),
         (STALEMATE, "f5f7", "Qf7")]


def test_bases(scamd, san, orc, dev):
    import scamd.fen
    # the oracle first: the expected words are python-chess's for these positions
    for fen, uci, word in BASED:
        assert cpu_game(orc, [orc.from_uci(uci)], fen) == [word], (fen, uci)
    st = orc.State(IN_CHECK)
    assert st.is_check() and len(st.legal_moves()) == 6
    st = orc.State(STALEMATE)
    st.push(orc.from_uci("f5f7"))
    assert st.legal_moves() == [] and not st.is_check()
    fens = [THREE_QUEENS, IN_CHECK, STALEMATE, BLACK_12]
    pos = scamd.fen.Positions(fens, 0).check()
    idx = {f: i for i, f in enumerate(fens)}
    games = [[orc.from_uci(u)] for _, u, _ in BASED]
    words, status, _ = run_write(scamd, san, dev, games, pos, [idx[f] for f, _, _ in BASED])
    assert status == [0] * len(BASED) and words == [[w] for _, _, w in BASED]
    # Black to move at move 12
    line = [orc.from_uci(u) for u in ("g8f6", "b1c3", "f8b4")]
    words, status, tok = run_write(scamd, san, dev, [line], pos, [idx[BLACK_12]])
    assert status == [0] and words == [cpu_game(orc, line, BLACK_12)] == [["Nf6", "Nc3", "Bb4"]]
    f = scamd.fen.parse_fen(BLACK_12)
    assert san.movetext(tok, f.fullmove, f.turn == 0) == "12... Nf6 13. Nc3 Bb4"
    # based games and games from the start position in one call: what the separate calls give
    plain = [[orc.from_uci(u) for u in ("e2e4", "e7e5", "g1f3")], [orc.from_uci("d2d4")]]
    mixed = [plain[0], games[0], games[1], plain[1], line, []]
    bidx = [-1, idx[THREE_QUEENS], idx[IN_CHECK], -1, idx[BLACK_12], idx[STALEMATE]]
    words, status, _ = run_write(scamd, san, dev, mixed, pos, bidx)
    alone, st_alone, _ = run_write(scamd, san, dev, plain)
    assert status == [0] * 6 and st_alone == [0, 0]
    assert words == [alone[0], ["Qh4e1"], ["Qh4xe1+"], alone[1], ["Nf6", "Nc3", "Bb4"], []]
    assert alone == [["e4", "e5", "Nf3"], ["d4"]]
    pos.close()


# ------------------------------------------------------------------ 4. failures
def test_failures_in_one_batch(scamd, san, orc, dev):
    u = lambda s: [orc.from_uci(x) for x in s.split()]
    clean = u("e2e4 e7e5 g1f3 b8c6 f1b5 a7a6")
    games = [clean,
             u("e2e5 e7e5"),                        # not legal at ply 0
             u("e2e4 e7e5 e1e3"),                   # ... at the last ply
             u("e2e4 e7e5 d1h6 g7h6 d2d4"),         # ... in the middle: the walk plays on, g7xh6 is legal where it arrives
             u("e2e4") + [0] + u("g1f3"),           # a move word of 0
             u("e2e4 e7e5 a3a4 d7d6"),              # a move from an empty square
             []]                                    # a game of 0 plies
    want = [0, -1, -3, -3, -2, -3, 0]
    words, status, tok = run_write(scamd, san, dev, games)
    assert status == want
    # the plies before the failing one are rendered, the tokens from it on are 0
    _, off = pack(games)
    for g, st in enumerate(want):
        good = len(games[g]) if st == 0 else -st - 1
        assert words[g] == cpu_game(orc, games[g][:good]), g
        assert (tok[off[g] + good:off[g + 1]] == 0).all(), g
    solo, st_solo, tok_solo = run_write(scamd, san, dev, [clean])
    assert st_solo == [0] and np.array_equal(tok[:len(clean)], tok_solo) and solo[0] == ["e4", "e5", "Nf3", "Nc6", "Bb5", "a6"]
    again = run_write(scamd, san, dev, games)
    assert again[1] == status and np.array_equal(again[2], tok)
    # a game of 4001 plies: refused by the return code, nothing is enqueued
    L = scamd.lib()
    d_tok, d_st = dev.alloc(4001 * 8), dev.alloc(16)
    rc = L.sc_moves_to_san_device(0, 1, _p(np.zeros(4001, np.uint16)), _p(np.array([0, 4001], np.uint32)), dev.stream, d_tok, d_st)
    assert rc == -1 and "too long" in L.sc_last_error().decode()
    dev.sync()
    assert (dev.read(d_tok, (4001,), np.uint64) == FILL64).all() and (dev.read(d_st, (4,), np.uint32) == FILL32).all()
    host = np.zeros(8, np.uint64)
    assert L.sc_moves_to_san_device(0, 1, _p(np.zeros(1, np.uint16)), _p(np.array([0, 1], np.uint32)), dev.stream, _p(host), d_st) == -1
    assert "tokens" in L.sc_last_error().decode() and "device memory" in L.sc_last_error().decode()


# ------------------------------------------------------------------ 5. batch edges
def test_batch_edges(scamd, san, orc, dev, golden, edge):
    L = scamd.lib()
    d_tok, d_st = dev.alloc(64), dev.alloc(64)
    assert L.sc_moves_to_san_device(0, 0, None, _p(np.zeros(1, np.uint32)), dev.stream, d_tok, d_st) == 0
    dev.sync()
    assert (dev.read(d_tok, (64,), np.uint8) == 0x5a).all() and (dev.read(d_st, (64,), np.uint8) == 0x5a).all()   # nothing is written
    assert run_write(scamd, san, dev, [[orc.from_uci("g1f3")]])[:2] == ([["Nf3"]], [0])
    # more games than lanes, lengths 0 .. the game's own: prefixes of the reference's games (a ply's word needs its own two positions only)
    cut = [(7 * i) % (len(golden["moves"][i % 60]) + 1) for i in range(65)]
    assert 0 in cut and max(cut) > 64
    words, status, _ = run_write(scamd, san, dev, [golden["moves"][i % 60][:cut[i]] for i in range(65)])
    assert status == [0] * 65 and words == [golden["words"][i % 60][:cut[i]] for i in range(65)]
    # the longest line alone: its last ply reads the record behind the last move
    k = max(range(90), key=lambda i: len(edge["moves"][i]))
    assert len(edge["moves"][k]) == 198
    assert run_write(scamd, san, dev, [edge["moves"][k]])[:2] == ([edge["words"][k]], [0])


def test_two_record_groups_long_game_in_the_first(scamd, san, orc, dev):
    """300 games of which game 150 has 4000 plies: 300 x 4002 position records exceed the walk's budget of 2^20, so the call
    walks two groups of games, the long game among short ones in the first"""
    u = lambda s: [orc.from_uci(x) for x in s.split()]
    short = [(u("e2e4 e7e5"), ["e4", "e5"]), (u("d2d4"), ["d4"]), (u("c2c4 c7c5 b1c3"), ["c4", "c5", "Nc3"])]
    games, want = [short[i % 3][0] for i in range(300)], [short[i % 3][1] for i in range(300)]
    games[150], want[150] = u("g1f3 g8f6 f3g1 f6g8") * 1000, ["Nf3", "Nf6", "Ng1", "Ng8"] * 1000
    assert len(games[150]) == 4000 and 262 * 4002 <= 2 ** 20 < 263 * 4002   # the first group ends behind game 261
    words, status, _ = run_write(scamd, san, dev, games)
    assert status == [0] * 300
    assert words == want


# ------------------------------------------------------------------ 6. the handle and the launcher
OPENING_FEN = "r1bqkbnr/pppp1ppp/2n5/4p3/4P3/5N2/PPPP1PPP/RNBQKB1R b KQkq - 2 3"
COMMON = [PLAY, "--white-device", "cuda", "--black-device", "cuda", "--black-type", "nn", "--rollout=12", "--temperature", "0",
          "--temperature-switch", "0", "--cpuct", "1.5", "--blocks", "1", "--channels", "128", "--white-seed", "3", "--black-seed", "4"]


def _play(out_dir, extra, pgn):
    os.makedirs(out_dir)
    r = subprocess.run(COMMON + ["-o", os.path.join(out_dir, "w_{}.json")] + [a.replace("@", out_dir) for a in extra] +
                       (["--pgn", os.path.join(out_dir, "match.pgn")] if pgn else []), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout


def _trace_moves(path):
    js = json.load(open(path))
    return js.get("opening", []) + [s[0] for s in js["steps"]], js


def _parse_back(scamd, san, dev, orc, games, fens):
    """movetext + FEN headers -> UCI moves per game, by the device parser (sc_encode_san_device_from: moves + status only)"""
    import scamd.fen
    L = scamd.lib()
    tokens, off = san.pack_tokens(games)
    n, P = len(games), int(off[-1])
    pos, bidx, owned = scamd.fen.bases_of(fens, n, 0)
    d_mv, d_st = dev.alloc(P * 2), dev.alloc(n * 4)
    rc = L.sc_encode_san_device_from(None, 0, n, pos.h if pos else None, _p(bidx) if pos else None, _p(tokens), _p(off), 0, 0, dev.stream,
                                     None, None, None, None, None, None, d_mv, d_st)
    assert rc == 0, L.sc_last_error().decode()
    dev.sync()
    if owned:
        pos.close()
    assert dev.read(d_st, (n,), np.int32).tolist() == [0] * n
    mv = dev.read(d_mv, (P,), np.uint16)
    return [[orc.uci(int(m)) for m in mv[off[g]:off[g + 1]]] for g in range(n)]


_RESULT = {"White": "1-0", "Black": "0-1", None: "1/2-1/2"}


def _headers(text):
    """per game of a PGN text: its tag pairs"""
    return [dict(re.findall(r'^\[(\w+) "(.*)"\]$', block, flags=re.M)) for block in re.split(r"\n\n(?=\[)", text.strip())]


SWAP = ["--games", "2", "--swap", "--swap-output", "@/b_{}.json", "--concurrency", "4", "--openings", "@/../suite.txt"]
SWAP_NAMES = ["w_1.json", "b_1.json", "w_2.json", "b_2.json"]       # handle order: game 2j + s is line j with the colours of set s


@pytest.fixture(scope="module")
def match(tmp_path_factory):
    """the launcher's runs, each made once: match("plain" | "swap", pgn) -> (directory, stdout)"""
    root = str(tmp_path_factory.mktemp("match"))
    with open(os.path.join(root, "suite.txt"), "w") as f:
        f.write("e2e4 c7c5 g1f3\nfen %s moves g8f6\n" % OPENING_FEN)
    done = {}

    def run(kind, pgn):
        if (kind, pgn) not in done:
            d = os.path.join(root, kind + ("_pgn" if pgn else ""))
            done[kind, pgn] = (d, _play(d, SWAP if kind == "swap" else ["--games", "6"], pgn))
        return done[kind, pgn]
    return run


def test_play_cli_pgn(scamd, san, orc, dev, match):
    """sc-play --pgn: the match as one PGN beside the JSON traces, which do not change"""
    (a, out), (a0, out0) = match("plain", True), match("plain", False)
    assert out == out0 and sorted(os.listdir(a0)) == ["w_%d.json" % k for k in range(1, 7)]            # no --pgn: today's output
    assert sorted(os.listdir(a)) == ["match.pgn"] + ["w_%d.json" % k for k in range(1, 7)]
    for k in range(1, 7):
        assert open(os.path.join(a, "w_%d.json" % k), "rb").read() == open(os.path.join(a0, "w_%d.json" % k), "rb").read()
    text = open(os.path.join(a, "match.pgn")).read()
    assert all(len(ln) <= 80 for ln in text.splitlines()) and text.endswith("\n\n")
    games, winners, fens = san.read_pgn(os.path.join(a, "match.pgn"), setup=True)
    tags = _headers(text)
    assert len(games) == len(tags) == 6 and fens == [None] * 6
    back = _parse_back(scamd, san, dev, orc, games, None)
    for k in range(6):
        moves, js = _trace_moves(os.path.join(a, "w_%d.json" % (k + 1)))
        assert back[k] == moves, k
        t = tags[k]
        assert (t["Round"], t["White"], t["Black"], t["Event"]) == (str(k), "net-seed3", "net-seed4", "sc-play match")
        assert t["Result"] == (_RESULT[js["outcome"]["winner"]] if js["outcome"] else "*")
        assert t.get("Termination") == (js["outcome"]["termination"] if js["outcome"] else None)
        assert games[k].split()[-1] == t["Result"] and "SetUp" not in t
        assert games[k].split()[:-1] == san.movetext(cpu_game(orc, [orc.from_uci(m) for m in moves])).split()   # the oracle's SAN


def test_play_cli_pgn_swap_and_openings(scamd, san, orc, dev, match):
    """both colour assignments on recycled slots, from a plain line and from a position, in one file"""
    (b, out), (b0, out0) = match("swap", True), match("swap", False)
    assert out == out0
    assert sorted(os.listdir(b0)) == sorted(SWAP_NAMES) and sorted(os.listdir(b)) == sorted(SWAP_NAMES + ["match.pgn"])
    for nm in SWAP_NAMES:
        assert open(os.path.join(b, nm), "rb").read() == open(os.path.join(b0, nm), "rb").read()
    text = open(os.path.join(b, "match.pgn")).read()
    games, winners, fens = san.read_pgn(os.path.join(b, "match.pgn"), setup=True)
    tags = _headers(text)
    assert len(games) == 4 and fens == [None, None, OPENING_FEN, OPENING_FEN]
    assert [("SetUp" in t, "FEN" in t) for t in tags] == [(False, False)] * 2 + [(True, True)] * 2
    assert [(t["White"], t["Black"]) for t in tags] == [("net-seed3", "net-seed4"), ("net-seed4", "net-seed3")] * 2
    assert games[0].startswith("1. e4 c5 2. Nf3 ") and games[1].startswith("1. e4 c5 2. Nf3 ")
    assert games[2].startswith("3... Nf6 4. ") and games[3].startswith("3... Nf6 4. ")
    back = _parse_back(scamd, san, dev, orc, games, fens)
    for k, nm in enumerate(SWAP_NAMES):
        moves, js = _trace_moves(os.path.join(b, nm))
        assert back[k] == moves and js.get("fen") == fens[k], nm
        assert tags[k]["Result"] == (_RESULT[js["outcome"]["winner"]] if js["outcome"] else "*")


@pytest.mark.parametrize("kind,pattern,order", [("plain", "w_*.json", (0, 1, 2, 3, 4, 5)), ("swap", "?_*.json", (1, 3, 0, 2))])
def test_trace_to_pgn_tool(san, match, kind, pattern, order):
    """the traces on disk -> PGN by the tool (a child process: it runs moves_to_san on torch's stream): the handle's movetext.
    order: the handle's game of every file, the files in the tool's (natural) order -- b_1, b_2, w_1, w_2 for the swapped match"""
    pytest.importorskip("torch")
    d, _ = match(kind, True)
    made = os.path.join(d, "tool.pgn")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "trace_to_pgn.py"), "-t", os.path.join(d, pattern), "-o", made],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    handle = san.read_pgn(os.path.join(d, "match.pgn"), setup=True)
    tool = san.read_pgn(made, setup=True)
    os.remove(made)
    for col in range(3):       # movetext, winner, FEN
        assert tool[col] == [handle[col][i] for i in order], col


def test_selfplay_handle_write_pgn(scamd, san, orc, tmp_path):
    """SelfPlay.write_pgn: nothing is written for a game that has not finished; then the chosen games in the chosen order, appended"""
    sp = scamd.SelfPlay(None, n_slots=4, n_games=4, rollout_num=16, num_steps=9, evaluator="synth", with_noise=False, seed=5)
    path = str(tmp_path / "games.pgn")
    with pytest.raises(scamd.EngineError) as err:
        sp.write_pgn([0], path)
    assert err.value.code == 1 and not os.path.exists(path)
    sp.run()
    sp.write_pgn([2, 0], path, white="new \"net\"", black="old", event="self-play")
    sp.write_pgn([1], path, append=True)
    text = open(path).read()
    games, winners, fens = san.read_pgn(path, setup=True)
    tags = _headers(text)
    assert len(games) == 3 and fens == [None] * 3 and text.endswith("\n\n")
    for k, g in enumerate((2, 0, 1)):
        tr = sp.trace(g)
        moves = [orc.from_uci(s[0]) if isinstance(s[0], str) else int(s[0]) for s in tr["steps"]]
        assert len(moves) == 9 and games[k].split()[:-1] == san.movetext(cpu_game(orc, moves)).split(), g
        assert tags[k]["Round"] == str(tr["game_id"]) and tags[k]["Result"] == games[k].split()[-1]
        assert tags[k]["Result"] == ("*" if tr["outcome"] is None else _RESULT[tr["outcome"]["winner"]])
    assert [(t["White"], t["Black"], t["Event"]) for t in tags] == [('new \\"net\\"', "old", "self-play")] * 2 + [("?", "?", "?")]
    with pytest.raises(scamd.EngineError):
        sp.write_pgn([4], path)                      # no such game
    sp.close()


# ------------------------------------------------------------------ torch
_CHILD = r'''
import json, sys
import torch                      # first: libsc_engine.so then binds to the runtime torch loaded
sys.path.insert(0, sys.argv[1])
import scamd
import scamd.san
job = json.load(open(sys.argv[2]))
torch.zeros(1, device="cuda:0")
with torch.cuda.stream(torch.cuda.Stream(0)):      # moves_to_san works on torch's current stream
    sans, status = scamd.san.moves_to_san(job["games"] + [["e2e4", "e7e5", "e1e3", "d7d6"], []])
    based, st2 = scamd.san.moves_to_san([["h4e1"], ["g1f3"]], fens=[job["fen"], None])
torch.cuda.synchronize()
print(json.dumps({"sans": sans, "status": status.tolist(), "based": based, "st2": st2.tolist()}))
'''


def test_moves_to_san_on_a_torch_stream(scamd, orc, golden, tmp_path):
    pytest.importorskip("torch")
    job = tmp_path / "job.json"
    job.write_text(json.dumps({"games": [[orc.uci(m) for m in g] for g in golden["moves"][:10]], "fen": THREE_QUEENS}))
    out = run_torch_child(tmp_path, _CHILD, os.path.join(ROOT, "smart-chess-rust_amd"), str(job), timeout=600)
    assert out["status"] == [0] * 10 + [-3, 0] and out["sans"] == golden["words"][:10] + [["e4", "e5"], []]
    assert out["st2"] == [0, 0] and out["based"] == [["Qh4e1"], ["Nf3"]]
