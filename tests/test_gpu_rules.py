"""GPU rules tests (-m gpu): the device's legal-move generator (gen_legal_wave, chess_rules_wave.hpp), its position updates
(make_move in k_encode_positions, make_move_board + k_ply_keys + k_ply_rep in the training-tensor encoder) and the in-tree rules
of the search, against the CPU oracle on positions chosen for being hard: the edge-case corpus (tests/golden/edge_lines.json)
on every ply and two plies below its final positions, games that play special moves whenever they can, and every position
four and five plies from the start (perft 4 and 5, known answers that do not depend on the oracle)."""
import ctypes as C
import random

import numpy as np
import pytest

from helpers import _same_tree, edge_features, load_edge_lines, mv_parts, random_games, random_steps, special_walk
from support import scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu
MAXC = 224
HIST_BUDGET = 512 << 20     # bytes of history scratch per sc_encode_positions call: n * (longest line + 2) * 80


@pytest.fixture(scope="module")
def eng(scamd):
    e = scamd.Engine(0, 128, seed=1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def idx_table(orc):
    """action index of every 16-bit move for each side to move, from the oracle: [turn][move] (-1 where unencodable)"""
    t = np.full((2, 1 << 15), -1, np.int32)
    for turn in (0, 1):
        for m in range(1 << 15):
            fr, to, p = mv_parts(m)
            if fr != to and p in (0, 2, 3, 4, 5):
                t[turn, m] = orc.move_index(m, turn)
    return t


def _encode(scamd, eng, lines, boards=True):
    """sc_encode_positions on move lists (lists of uint16), chunked so that one call's history scratch stays under HIST_BUDGET;
    legal-move tables come back padded (rows zero past n_legal)"""
    L = scamd.lib()
    n = len(lines)
    out = dict(n_legal=np.zeros(n, np.int32), lm=np.zeros((n, MAXC), np.uint16), li=np.zeros((n, MAXC), np.uint16),
               meta=np.zeros((n, 7), np.int32), oc=np.zeros((n, 4), np.int32))
    if boards:
        out["boards"] = np.zeros((n, 8, 8, 112), np.int8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    a = 0
    while a < n:
        e, longest = a, 0
        while e < n and (e - a + 1) * (max(longest, len(lines[e])) + 2) * 80 <= HIST_BUDGET and e - a < 32768:
            longest = max(longest, len(lines[e]))
            e += 1
        off = np.zeros(e - a + 1, np.uint32)
        off[1:] = np.cumsum([len(x) for x in lines[a:e]])
        flat = np.asarray([m for x in lines[a:e] for m in x] or [0], np.uint16)
        rc = L.sc_encode_positions(eng.h, 0, e - a, p(flat), p(off), p(out["boards"][a:e]) if boards else None, p(out["meta"][a:e]),
                                   p(out["lm"][a:e]), p(out["li"][a:e]), p(out["n_legal"][a:e]), p(out["oc"][a:e]))
        assert rc == 0, scamd.lib().sc_last_error()
        a = e
    return out


class _Expect:
    """the oracle's answers for a batch of positions, gathered while walking the oracle State"""

    def __init__(self):
        self.lines, self.boards, self.meta, self.legal, self.check, self.term, self.winner = [], [], [], [], [], [], []

    def add(self, line, st, boards=True):
        self.lines.append(list(line))
        if boards:
            b, m = st.encode()
            self.boards.append(b)
            self.meta.append(m)
        self.legal.append(st.legal_moves())
        self.check.append(st.is_check())
        oc = st.outcome()
        self.term.append(oc["termination"] if oc else None)
        self.winner.append(oc["winner"] if oc else None)


def _compare(scamd, eng, idx_table, ex, what):
    """device == oracle on every position of ex: boards, meta, legal moves in order, legal_idx, is_check, termination, winner,
    status -> the device's n_legal"""
    r = _encode(scamd, eng, ex.lines)
    n = len(ex.lines)
    want = np.zeros((n, MAXC), np.uint16)
    nl = np.array([len(x) for x in ex.legal], np.int32)
    for i, x in enumerate(ex.legal):
        want[i, :len(x)] = x
    turn = np.array([int(m[0]) for m in ex.meta], np.int64)
    want_idx = np.where(np.arange(MAXC)[None, :] < nl[:, None], idx_table[turn[:, None], want], 0)
    for i in np.flatnonzero((r["lm"] != want).any(1) | (r["n_legal"] != nl))[:1]:
        pytest.fail(f"{what}: legal moves differ at {[scamd.move_uci(m) for m in ex.lines[i]]}: device "
                    f"{[scamd.move_uci(m) for m in r['lm'][i, :r['n_legal'][i]]]} oracle {[scamd.move_uci(m) for m in ex.legal[i]]}")
    assert (want_idx >= 0).all() and np.array_equal(r["li"].astype(np.int32), want_idx), what
    bad = np.flatnonzero(~(r["boards"] == np.stack(ex.boards)).reshape(n, -1).all(1) | ~(r["meta"] == np.stack(ex.meta)).all(1))
    assert bad.size == 0, (what, [scamd.move_uci(m) for m in ex.lines[bad[0]]])
    assert r["oc"][:, 2].astype(bool).tolist() == ex.check, what
    assert [scamd.TERMINATION[int(t)] for t in r["oc"][:, 0]] == ex.term, what
    for i in np.flatnonzero([t is not None for t in ex.term]):
        assert {1: "White", 0: "Black", -1: None}[int(r["oc"][i, 1])] == ex.winner[i], (what, i)
    assert (r["oc"][:, 3] == 0).all(), what
    return r["n_legal"]


def _perft_lines(orc, depth):
    """every line of exactly `depth` plies from the start, in the oracle's move order, and the padded legal-move rows of their
    final positions"""
    lines, rows = [], []
    st = orc.State()
    path = []

    def rec(d):
        lm = st.legal_moves()
        if d == depth:
            lines.append(list(path))
            rows.append(lm)
            return
        for m in lm:
            st.push(m)
            path.append(m)
            rec(d + 1)
            path.pop()
            st.pop()
    rec(0)
    return lines, rows


def test_device_perft_from_start(scamd, orc, eng, idx_table):
    """every position 3 and 4 plies from the start through gen_legal_wave: the n_legal sums are perft(4) and perft(5), and every
    legal-move row (its order too) and action-index row equals the oracle's"""
    for depth, want_sum, want_n in ((3, 197281, 8902), (4, 4865609, 197281)):
        lines, rows = _perft_lines(orc, depth)
        assert len(lines) == want_n
        r = _encode(scamd, eng, lines, boards=False)
        assert int(r["n_legal"].sum()) == want_sum, depth
        assert (r["oc"][:, 3] == 0).all()
        turn = 1 - (depth & 1)
        for a in range(0, want_n, 32768):   # padded arrays, a slice at a time
            e = min(a + 32768, want_n)
            nl = np.array([len(x) for x in rows[a:e]], np.int32)
            want = np.zeros((e - a, MAXC), np.uint16)
            for i, x in enumerate(rows[a:e]):
                want[i, :len(x)] = x
            assert np.array_equal(r["n_legal"][a:e], nl), depth
            bad = np.flatnonzero((r["lm"][a:e] != want).any(1))
            assert bad.size == 0, (depth, [scamd.move_uci(m) for m in lines[a + bad[0]]])
            want_idx = np.where(np.arange(MAXC)[None, :] < nl[:, None], idx_table[turn][want], 0)
            assert (want_idx >= 0).all() and np.array_equal(r["li"][a:e].astype(np.int32), want_idx), depth


def _corpus_moves(orc):
    return [(e, [orc.from_uci(u) for u in e["uci"]]) for e in load_edge_lines()]


def test_edge_lines_every_ply(scamd, orc, eng, idx_table):
    """every prefix of every corpus line: planes, meta, legal moves in order, action indices, check flag, termination, winner"""
    ex = _Expect()
    for e, moves in _corpus_moves(orc):
        st = orc.State()
        for i in range(len(moves) + 1):
            ex.add(moves[:i], st)
            if i < len(moves):
                st.push(moves[i])
    assert len(ex.lines) > 4000
    _compare(scamd, eng, idx_table, ex, "corpus prefixes")


def test_edge_positions_depth2_subtrees(scamd, orc, eng, idx_table):
    """every line of depth <= 2 below each corpus final position, with the same comparisons; the n_legal sum over the depth-2
    leaves is the oracle's perft(3) there"""
    total = 0
    for e, moves in _corpus_moves(orc):
        st = orc.State()
        for m in moves:
            st.push(m)
        if st.outcome():
            continue
        ex = _Expect()
        leaves = []
        ex.add(moves, st)
        for a in st.legal_moves():
            st.push(a)
            ex.add(moves + [a], st)
            for b in st.legal_moves():
                st.push(b)
                leaves.append(len(ex.lines))
                ex.add(moves + [a, b], st)
                st.pop()
            st.pop()
        nl = _compare(scamd, eng, idx_table, ex, e["name"])
        assert int(nl[leaves].sum()) == st.perft(3), e["name"]
        total += len(ex.lines)
    assert total > 30000


def test_every_ply_of_special_move_games(scamd, orc, eng, idx_table):
    """240 games that play en passant, castling, promotions and checks whenever they can (a quarter of them opening with a corpus
    line that ends at an en-passant capture), every ply against the oracle; the predicates count what was covered"""
    starts = [[orc.from_uci(u) for u in e["uci"]] for e in load_edge_lines()
              if e["category"] in ("ep_pin_horizontal", "ep_pin_diagonal", "ep_pinned_along_pin", "ep_discovered_check",
                                   "rep_dp_ep_pinned", "ep_two_capturers", "ep_evades_pawn_check")]
    games = special_walk(orc, 180, 200, seed=21) + special_walk(orc, 60, 200, seed=22, starts=starts)
    ex = _Expect()
    cover = dict(positions=0, ep=0, ep_pinned=0, castling=0, promotion=0)
    for gi, (moves, _) in enumerate(games):
        st = orc.State()
        for i in range(len(moves) + 1):
            ex.add(moves[:i], st)
            f = edge_features(st, moves[i - 1] if i else None, repetition=False)
            lm = ex.legal[-1]
            cover["ep"] += "ep_legal" in f
            cover["ep_pinned"] += bool(f & {"ep_pin_horizontal", "ep_pin_diagonal"})
            cover["castling"] += any(abs(st.piece_at(m & 63)) == 6 and abs(((m >> 6) & 63) - (m & 63)) == 2 for m in lm)
            cover["promotion"] += any(m >> 12 for m in lm)
            if i < len(moves):
                st.push(moves[i])
        if len(ex.lines) > 8000 or gi == len(games) - 1:   # keeps the oracle's planes for one batch at a time in memory
            _compare(scamd, eng, idx_table, ex, "special-move games")
            cover["positions"] += len(ex.lines)
            ex = _Expect()
    print("coverage", cover)
    assert cover["positions"] >= 30000, cover
    assert cover["ep"] >= 200 and cover["ep_pinned"] >= 20 and cover["castling"] >= 200 and cover["promotion"] >= 100, cover


@pytest.mark.parametrize("mirror", [False, True])
def test_encode_steps_on_edge_lines(scamd, orc, mirror):
    """every corpus line (and one more ply where the game goes on) as a game in one sc_encode_steps batch with random games:
    planes, meta, dist (as uint32), move indices bit for bit against the oracle; the three repetition-across-a-double-push
    kinds set the repetition planes exactly as the oracle does (make_move_board -> k_ply_keys -> k_ply_rep)"""
    rnd = random.Random(4)
    games, names = [], []
    for e, moves in _corpus_moves(orc):
        st = orc.State()
        for m in moves:
            st.push(m)
        lm = st.legal_moves()
        games.append(moves + ([lm[0]] if lm else []))
        names.append(e["category"])
    games += [g for g, _ in random_games(orc, 30, 150, seed=8) if g]
    names += ["random"] * (len(games) - len(names))
    steps = [random_steps(orc, g, rnd) for g in games]   # children: the legal moves shuffled, counts 0..200
    r = scamd.encode_steps_batch(steps, mirror)
    assert (r["status"] == 0).all()
    off = r["ply_off"]
    last = {}
    for gi, st in enumerate(steps):
        rc, b, m, d, idx = orc.encode_steps(st, mirror)
        assert rc == 0
        a, e = int(off[gi]), int(off[gi + 1])
        assert (r["boards"][a:e] == b).all(), (gi, names[gi])
        assert (r["meta"][a:e] == m).all(), (gi, names[gi])
        assert (r["dist"][a:e].view(np.uint32) == d.view(np.uint32)).all(), (gi, names[gi])
        for k in range(e - a):
            assert (r["move_indices"][a + k] == idx[k]).all(), (gi, k)
        last.setdefault(names[gi], []).append((b[-1][:, :, 12].all(), b[-1][:, :, 13].all()))
    # the final position of each line (encoded as the extra ply): repeated three / five times after a plain or pinned-ep double
    # push -> both planes; the same board after a legal-ep double push -> not the same position, only the later repeat
    assert last["rep_dp_plain_3"] == last["rep_dp_plain_5"] == last["rep_dp_ep_pinned"] == [(True, True)] * 2
    assert last["rep_dp_legal_ep"] == [(True, False)] * 2


def _lockstep_lines(orc):
    """corpus positions with en passant, castling, promotion, double check, a mate in one and a threefold claim within the first
    plies of a search tree"""
    by = {}
    for e in load_edge_lines():
        by.setdefault(e["category"], []).append(e["uci"])
    pick = lambda c: min(by[c], key=len)

    def before_the_end(line):   # the longest prefix whose game is not over yet (a claimable draw ends it too)
        st = orc.State()
        for m in line:
            st.push(m)
        while st.outcome() is not None:
            st.pop()
            line = line[:-1]
        return line
    return [pick("ep_legal"), pick("ep_two_capturers"), pick("castle_both"), pick("promo_push_all_four"), pick("double_check"),
            pick("promo_captures_checker"), before_the_end(pick("checkmate")), before_the_end(pick("threefold"))]


@pytest.mark.parametrize("k", range(8))
def test_search_lockstep_from_edge_positions(scamd, orc, k):
    """the search from corpus positions (k_set_position, make_move and position_key_wave in the tree, in-tree repetition flags):
    every 7th and the last simulations, identical node pool and path to the oracle's search (test_search_lockstep_exact's
    protocol)"""
    line = _lockstep_lines(orc)[k]
    R = 120
    sp = scamd.SelfPlay(None, n_slots=2, n_games=2, rollout_num=R, num_steps=20, cpuct=2.5, with_noise=False,
                        evaluator="synth", seed=3)
    st = orc.State()
    for m in line:
        st.push(m)
    assert st.outcome() is None and st.legal_moves()
    sp.set_position(0, line)
    srch = orc.Search(st)
    for s in range(R - 1):
        sp.enqueue(1)
        srch.sim(cpuct=2.5, with_noise=False)
        if s % 7 == 0 or s > R - 5:
            t, d = sp.tree(0), srch.dump()
            assert _same_tree(t, d), s
            assert list(sp.slot(0)["path"]) == list(srch.last_path())
    assert sp.stats()["error_flags"] == 0
    sp.close()


def _replay_lines(orc):
    """three lines for the replay step k_set_position and k_encode_positions share: under 8 plies; a corpus line cut one move
    before its threefold repetition; 81 plies whose last position is the one after ply 1 -- 1. a4, then the g1 knight walks a
    cycle of 8 squares and the b8 knight one of 10, which meet again after 40 moves each -- so the repeated position lies 80
    plies back and the scan's second round of 64 lanes finds it"""
    short = [orc.from_uci(u) for u in ("e2e4", "c7c5", "g1f3")]
    three = [orc.from_uci(u) for u in min((e["uci"] for e in load_edge_lines() if e["category"] == "threefold"), key=len)]
    st = orc.State()
    for m in three:
        st.push(m)
    while st.is_repetition(3):
        st.pop()
        three = three[:-1]
    assert any(_pushed_rep3(st, m) for m in st.legal_moves())
    wn = ["g1", "f3", "d4", "f5", "g3", "e4", "g5", "h3"]
    bn = ["b8", "a6", "c5", "e6", "f4", "g6", "e5", "c4", "a5", "c6"]
    long = ["a2a4"]
    for k in range(40):
        long += [bn[k % 10] + bn[(k + 1) % 10], wn[k % 8] + wn[(k + 1) % 8]]
    long = [orc.from_uci(u) for u in long]
    for line, rep2 in ((short, False), (three, True), (long, True)):
        st = orc.State()
        for m in line:
            assert m in st.legal_moves()
            st.push(m)
        assert st.legal_moves() and st.is_repetition(2) == rep2 and not st.is_repetition(3)
        # (the oracle's outcome claims the draw one move early, python-chess can_claim_threefold_repetition: the search goes on)
        assert st.outcome() == (dict(termination="ThreefoldRepetition", winner=None) if line is three else None)
    assert len(short) < 8 and len(long) == 81
    return [short, three, long]


def _pushed_rep3(st, m):
    st.push(m)
    r = st.is_repetition(3)
    st.pop()
    return r


@pytest.mark.parametrize("k", range(3))
def test_replay_step_callers_agree(scamd, orc, eng, idx_table, k):
    """replay_step (position_chain.hpp) through both of its callers on the same line: sc_encode_positions -- planes, meta, legal
    moves, action indices, outcome -- equals the oracle; the slot sc_selfplay_set_position fills has the line's ply, the oracle's
    legal moves as the root's children after one simulation (the row sc_encode_positions gave), and searches in lockstep with
    the oracle from there (the long line: leaves 64 plies and more from the repeated position)"""
    line = _replay_lines(orc)[k]
    st = orc.State()
    for m in line:
        st.push(m)
    ex = _Expect()
    ex.add(line, st)
    r = _encode(scamd, eng, [line])
    nl = _compare(scamd, eng, idx_table, ex, "replay line %d" % k)
    R = 60
    sp = scamd.SelfPlay(None, n_slots=2, n_games=2, rollout_num=R, num_steps=20, cpuct=2.5, with_noise=False,
                        evaluator="synth", seed=3)
    sp.set_position(0, line)
    s0 = sp.slot(0)
    assert (s0["ply"], s0["sim"], s0["status"]) == (len(line), 0, 1)
    srch = orc.Search(st)
    for s in range(R - 1):
        sp.enqueue(1)
        srch.sim(cpuct=2.5, with_noise=False)
        if s % 7 == 0 or s > R - 5:
            t, d = sp.tree(0), srch.dump()
            assert _same_tree(t, d), s
            assert list(sp.slot(0)["path"]) == list(srch.last_path())
        if s == 0:
            assert t["n_child"][0] == nl[0] == len(ex.legal[0])
            assert list(t["move"][1:1 + nl[0]]) == list(r["lm"][0, :nl[0]]) == list(ex.legal[0])
    assert sp.stats()["error_flags"] == 0
    sp.close()
