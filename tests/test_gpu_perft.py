"""Perft on the device (-m gpu; no torch in the process): sc_perft's node counts, kinds and divide against the table of expected
values (tests/perft_ref.py), the published deep totals, the CPU oracle's perft and legal moves, and the Python yardstick; the
same bytes at every max_frontier; many roots; the edge-case corpus; the edges of the interface; scamd.rules and tools/perft.py."""
import ctypes as C

import numpy as np
import pytest

import perft_ref
from helpers import load_edge_lines
from support import _p, scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu
ROW = 224
STALEMATE = "7k/5Q2/6K1/8/8/8/8/8 b - - 0 1"
MATED = "R5k1/5ppp/8/8/8/8/8/6K1 b - - 0 1"


@pytest.fixture(scope="module")
def fen(scamd):
    import scamd.fen as m
    return m


@pytest.fixture(scope="module")
def rules(scamd):
    import scamd.rules as m
    return m


def run(scamd, fen, entries, depth, max_frontier=0, kinds=True, divide=True, n_div=True, status=True, guard=0, expect=0):
    """sc_perft on entries [(FEN or None, [moves as uint16 or UCI])] -> the raw output arrays (dict), each `guard` rows longer at
    both ends than the call may touch and pre-filled with 0x5a"""
    L = scamd.lib()
    n = len(entries)
    texts = [f for f, _ in entries if f is not None]
    pos = fen.Positions(texts) if texts else None
    bidx, k = np.full(max(n, 1), -1, np.int32), 0
    for i, (f, _) in enumerate(entries):
        if f is not None:
            bidx[i], k = k, k + 1
    ml = [[scamd.uci_move(m) if isinstance(m, str) else int(m) for m in mv] for _, mv in entries]
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum([len(g) for g in ml])
    flat = np.asarray([m for g in ml for m in g] or [0], np.uint16)

    def buf(cols, dtype, want=True):
        if not want:
            return None
        a = np.empty((n + 2 * guard, cols) if cols else (n + 2 * guard,), dtype)
        a.view(np.uint8)[...] = 0x5a
        return a

    full = dict(nodes=buf(0, np.uint64), kinds=buf(8, np.uint64, kinds), div_moves=buf(ROW, np.uint16, divide), div_nodes=buf(ROW, np.uint64, divide),
                n_div=buf(0, np.int32, n_div), status=buf(0, np.int32, status))
    ptr = {k: (None if a is None else C_ptr(a, guard)) for k, a in full.items()}
    try:
        rc = L.sc_perft(0, n, pos.h if pos is not None else None, _p(bidx) if pos is not None else None, _p(flat), _p(off), depth, max_frontier,
                        ptr["nodes"], ptr["kinds"], ptr["div_moves"], ptr["div_nodes"], ptr["n_div"], ptr["status"])
    finally:
        if pos is not None:
            pos.close()
    assert rc == expect, (rc, L.sc_last_error().decode())
    out = {}
    for k, a in full.items():
        if a is None:
            continue
        if guard:
            edge = np.concatenate([a[:guard].reshape(-1).view(np.uint8), a[guard + n:].reshape(-1).view(np.uint8)])
            assert (edge == 0x5a).all(), k
        out[k] = a[guard:guard + n]
    return out


def C_ptr(a, guard):
    """the address of row `guard` of a"""
    return C.c_void_p(a.ctypes.data + guard * a.strides[0])


def _columns(r, i):
    return (int(r["nodes"][i]),) + tuple(int(v) for v in r["kinds"][i, 1:7])


def _divide(r, i):
    k = int(r["n_div"][i])
    return [(int(r["div_moves"][i, j]), int(r["div_nodes"][i, j])) for j in range(k)]


def _check_rows(r, i):
    """what holds for every entry: slot 0 repeats the nodes, slot 7 is 0, rows are zero from n_div on and sum to the nodes"""
    k = int(r["n_div"][i])
    assert int(r["kinds"][i, 0]) == int(r["nodes"][i]) and int(r["kinds"][i, 7]) == 0
    assert not r["div_moves"][i, k:].any() and not r["div_nodes"][i, k:].any()
    assert int(r["div_nodes"][i].sum()) == int(r["nodes"][i])


# ---------------------------------------------------------------------------------- 1. the table
@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5])
def test_table(scamd, fen, orc, depth):
    """one call per depth with every position that has that depth, kinds and divide on: every column the table has; for rows of at
    most about 10^5 nodes the divide is the oracle's (push(m); perft(depth - 1)), move for move and in order"""
    fens = [f for f, rows in perft_ref.TABLE.items() if depth in rows]
    r = run(scamd, fen, [(f, []) for f in fens], depth)
    assert not r["status"].any()
    for i, f in enumerate(fens):
        want = perft_ref.TABLE[f][depth]
        got = _columns(r, i)
        print(f, depth, got)
        assert [g for g, w in zip(got, want) if w is not None] == [w for w in want if w is not None], (f, got)
        _check_rows(r, i)
        st = orc.State(f)
        assert [m for m, _ in _divide(r, i)] == st.legal_moves()
        if want[0] <= perft_ref.SMALL:
            assert _divide(r, i) == perft_ref.divide_by_oracle(st, depth), f


# ---------------------------------------------------------------------------------- 2. deep totals
@pytest.mark.parametrize("case", perft_ref.DEEP, ids=["start-d6", "kiwipete-d5", "pos3-d6"])
def test_deep_totals(scamd, fen, case):
    """published node totals, nodes only, at the default max_frontier: the start position's last built level has 4.87 M nodes, so
    a level outgrows its buffer of 2^20 and is walked in pieces"""
    f, depth, want = case
    r = run(scamd, fen, [(f, [])], depth, kinds=False, divide=False, n_div=False)
    print(f, depth, int(r["nodes"][0]))
    assert int(r["nodes"][0]) == want and int(r["status"][0]) == 0


# ---------------------------------------------------------------------------------- 3. no output depends on the capacity
def test_capacity_independence(scamd, fen):
    for f, depth in ((perft_ref.KIWI, 3), (perft_ref.POS4, 4)):
        outs = [run(scamd, fen, [(f, [])], depth, max_frontier=mf) for mf in (256, 1000, 1 << 20)]
        assert _columns(outs[0], 0) == perft_ref.TABLE[f][depth]
        for o in outs[1:]:
            for k in outs[0]:
                assert o[k].tobytes() == outs[0][k].tobytes(), (f, k)


def test_refused_capacities_and_depths(scamd, fen):
    L = scamd.lib()
    for mf in (255, (1 << 24) + 1):
        r = run(scamd, fen, [(None, [])], 1, max_frontier=mf, guard=1, expect=-1)
        assert "max_frontier" in L.sc_last_error().decode() and (r["nodes"].view(np.uint8) == 0x5a).all()
    for depth in (-1, 17):
        r = run(scamd, fen, [(None, [])], depth, guard=1, expect=-1)
        assert "depth" in L.sc_last_error().decode() and (r["nodes"].view(np.uint8) == 0x5a).all()


# ---------------------------------------------------------------------------------- 4. many roots
def test_many_roots(scamd, fen, orc):
    """the 8 902 positions three plies from the start as 8 902 entries, at max_frontier 256: the roots are cut into 35 pieces and
    each piece's children again.  nodes[i] is the oracle's perft(2) there, the sum is perft(5), and the depth-1 divide rows are the
    oracle's legal moves in order"""
    st, lines, want2, legal = orc.State(), [], [], []

    def rec(line):
        if len(line) == 3:
            lines.append(list(line))
            want2.append(st.perft(2))
            legal.append(st.legal_moves())
            return
        for m in st.legal_moves():
            st.push(m)
            rec(line + [m])
            st.pop()

    rec([])
    assert len(lines) == 8902
    entries = [(None, ln) for ln in lines]
    r = run(scamd, fen, entries, 2, max_frontier=256)
    assert not r["status"].any()
    assert r["nodes"].tolist() == want2 and int(r["nodes"].sum()) == 4865609
    for i in (0, 4451, 8901):
        _check_rows(r, i)
    assert r["div_nodes"].sum(axis=1).tolist() == want2
    r1 = run(scamd, fen, entries, 1, max_frontier=256)
    assert r1["n_div"].tolist() == [len(x) for x in legal] == r1["nodes"].tolist()
    for i, lm in enumerate(legal):
        assert r1["div_moves"][i, :len(lm)].tolist() == lm, i
    assert (r1["div_nodes"] == (np.arange(ROW)[None, :] < r1["n_div"][:, None])).all()
    assert (r["div_moves"] == r1["div_moves"]).all()


# ---------------------------------------------------------------------------------- 5. the edge corpus
def test_edge_corpus(scamd, fen, orc):
    """the 90 final positions of tests/golden/edge_lines.json as move lists in one call: depth 2 with kinds is the yardstick's,
    depth 3 nodes are State.perft(3) -- also where a draw could be claimed: the walk goes on there"""
    corpus = load_edge_lines()
    assert len(corpus) == 90
    entries = [(None, e["uci"]) for e in corpus]
    r2 = run(scamd, fen, entries, 2)
    r3 = run(scamd, fen, entries, 3, kinds=False, divide=False, n_div=False)
    assert not r2["status"].any() and not r3["status"].any()
    claimable = 0
    for i, e in enumerate(corpus):
        st = orc.State()
        for u in e["uci"]:
            st.push(u)
        ref = perft_ref.perft(st, 2)
        assert _columns(r2, i) == (ref["nodes"],) + tuple(ref["kinds"]), e["name"]
        assert _divide(r2, i) == ref["divide"], e["name"]
        _check_rows(r2, i)
        assert int(r3["nodes"][i]) == st.perft(3), e["name"]
        claimable += int(st.outcome() is not None and bool(st.legal_moves()))
    assert claimable > 0


# ---------------------------------------------------------------------------------- 6. edges
def test_depth_zero_and_one(scamd, fen, orc):
    """depth 0: one node, no kinds, no divide; depth 1: the legal_moves rows and n_legal of sc_encode_positions_from for the same
    entries"""
    entries = [(perft_ref.KIWI, []), (None, ["e2e4", "c7c5"]), (perft_ref.POS5, ["d7c8q"]), (MATED, [])]
    r0 = run(scamd, fen, entries, 0, guard=2)
    assert r0["nodes"].tolist() == [1] * 4 and not r0["kinds"][:, 1:].any() and r0["kinds"][:, 0].tolist() == [1] * 4
    assert not r0["n_div"].any() and not r0["div_moves"].any() and not r0["div_nodes"].any() and not r0["status"].any()
    r1 = run(scamd, fen, entries, 1, guard=2)
    enc = scamd.encode_positions([m for _, m in entries], fens=[f for f, _ in entries])
    assert r1["n_div"].tolist() == enc["n_legal"].tolist() == r1["nodes"].tolist()
    for i in range(4):
        assert r1["div_moves"][i, :r1["n_div"][i]].tolist() == enc["legal_moves"][i].tolist()
        _check_rows(r1, i)
    assert _columns(r1, 0) == perft_ref.TABLE[perft_ref.KIWI][1]


def test_roots_without_moves(scamd, fen):
    """a mated and a stalemated root (bases of status 1 are accepted): nothing at any depth >= 1"""
    for depth in (1, 2, 3):
        r = run(scamd, fen, [(MATED, []), (perft_ref.KIWI, []), (STALEMATE, [])], depth, guard=1)
        assert r["nodes"].tolist()[::2] == [0, 0] and r["n_div"].tolist()[::2] == [0, 0] and not r["kinds"][::2].any()
        assert not r["div_moves"][::2].any() and not r["div_nodes"][::2].any() and not r["status"].any()
        assert _columns(r, 1) == perft_ref.TABLE[perft_ref.KIWI][depth]


def test_wide_position(scamd, fen, orc):
    """218 legal moves: more than three passes of 64 lanes in the expansion and in the classification"""
    st = orc.State(perft_ref.WIDE)
    r1 = run(scamd, fen, [(perft_ref.WIDE, [])], 1)
    assert int(r1["n_div"][0]) == 218 and r1["div_moves"][0, :218].tolist() == st.legal_moves()
    for depth in (1, 2, 3):
        r = run(scamd, fen, [(perft_ref.WIDE, [])], depth, max_frontier=256 if depth == 3 else 0)
        ref = perft_ref.perft(st, depth)
        assert _columns(r, 0) == (ref["nodes"],) + tuple(ref["kinds"]) and _divide(r, 0) == ref["divide"]
    assert int(r["nodes"][0]) == 19073


def _absent_move(st):
    """a from-to pair that none of st's legal moves has"""
    pairs = {m & 0xfff for m in st.legal_moves()}
    return next(m for m in range(1, 4096) if (m & 63) != (m >> 6) and m not in pairs)


def test_the_move_lookup_at_every_round_of_the_legal_list(scamd, fen, orc):
    """the 218 moves of WIDE fill three rounds of 64 lanes and 26 lanes of a fourth: one-move lines through the first and last move
    of every round, a move that is in no round, and an absent move behind a legal one, through the three callers of the lookup
    that take move lists -- the position encoder, the opening lines of a match handle and perft's roots"""
    root = orc.State(perft_ref.WIDE)
    legal = root.legal_moves()
    assert len(legal) == 218
    lines = [[legal[k]] for k in (0, 63, 64, 127, 128, 191, 192, 217)]
    after = []
    for ln in lines:
        st = root.copy()
        st.push(ln[0])
        after.append(st)
    lines += [[_absent_move(root)], [legal[0], _absent_move(after[0])]]
    fens = [perft_ref.WIDE] * 10
    enc = scamd.encode_positions(lines, fens=fens)
    assert enc["status"].tolist() == [0] * 8 + [-1, -2]
    for i, st in enumerate(after):
        ob, om = st.encode()
        assert np.array_equal(enc["boards"][i], ob) and np.array_equal(enc["meta"][i], om), i
        assert enc["legal_moves"][i].tolist() == st.legal_moves(), i
    sp = scamd.SelfPlay(None, evaluator="synth", seed=5, with_noise=False, outcome_gate=-1, rollout_num=20, n_slots=2, n_games=2, num_steps=3)
    sp.set_match(None, None, 11, 22, colours=1)
    with pytest.raises(scamd.EngineError) as e:
        sp.set_openings(list(zip(fens, lines)))
    sp.close()
    over = [int(st.outcome() is not None or not st.legal_moves()) for st in after]
    assert e.value.code == -1 and e.value.status == over + [-1, -2]
    r = run(scamd, fen, list(zip(fens, lines)), 1, guard=1)
    assert r["status"].tolist() == [0] * 8 + [-1, -2]
    assert r["nodes"].tolist() == [st.perft(1) for st in after] + [0, 0]
    for i, st in enumerate(after):
        assert r["div_moves"][i, :r["n_div"][i]].tolist() == st.legal_moves(), i


def test_mixed_entries_and_an_illegal_move(scamd, fen, orc):
    """FEN bases, the start position (base_idx -1) and move lists in one call; an illegal move in one list gives -(j+1) there and
    leaves its neighbours as they are without it"""
    good = [(perft_ref.KIWI, ["e1g1", "e8c8"]), (None, ["e2e4", "e7e5", "g1f3"]), (perft_ref.POS3, []), (None, []), (perft_ref.POS4, ["c4c5"])]
    bad = list(good)
    bad[1] = (None, ["e2e4", "e7e5", "e1e3"])          # move 2 is not legal
    bad[4] = (perft_ref.POS4, ["c4c5", "e8g8"])        # g8 is attacked by the knight on h6: move 1
    a, b = run(scamd, fen, good, 3, guard=1), run(scamd, fen, bad, 3, guard=1)
    assert a["status"].tolist() == [0] * 5 and b["status"].tolist() == [0, -3, 0, 0, -2]
    for i, (f, mv) in enumerate(good):
        st = orc.State(f) if f else orc.State()
        for u in mv:
            st.push(u)
        ref = perft_ref.perft(st, 3)
        assert _columns(a, i) == (ref["nodes"],) + tuple(ref["kinds"]) and _divide(a, i) == ref["divide"], i
    for i in (0, 2, 3):
        for k in a:
            assert a[k][i].tobytes() == b[k][i].tobytes(), (i, k)
    for i in (1, 4):
        assert int(b["nodes"][i]) == 0 and int(b["n_div"][i]) == 0 and not b["kinds"][i].any()
        assert not b["div_moves"][i].any() and not b["div_nodes"][i].any()


def test_a_refused_base_refuses_the_call(scamd, fen):
    """a base of negative status: -1 and nothing is written"""
    r = run(scamd, fen, [(perft_ref.KIWI, []), ("8/8/8/8/8/8/8/Kk6 w - - 0 1", [])], 2, guard=1, expect=-1)
    assert "status -3" in scamd.lib().sc_last_error().decode()
    for k, a in r.items():
        assert (a.reshape(-1).view(np.uint8) == 0x5a).all(), k


def test_no_entries_and_null_outputs(scamd, fen):
    """n == 0; each optional pointer NULL in turn gives the other outputs unchanged; two identical calls give identical bytes"""
    run(scamd, fen, [], 3, guard=1)
    entries = [(perft_ref.POS4, []), (None, ["d2d4"]), (perft_ref.QUEEN_MATE, [])]
    full = run(scamd, fen, entries, 3, guard=1)
    again = run(scamd, fen, entries, 3, guard=1)
    for k in full:
        assert full[k].tobytes() == again[k].tobytes(), k
    for skip in ("kinds", "divide", "n_div", "status"):
        r = run(scamd, fen, entries, 3, guard=1, **{skip: False})
        for k in r:
            assert r[k].tobytes() == full[k].tobytes(), (skip, k)
    r = run(scamd, fen, entries, 3, guard=1, kinds=False, divide=False, n_div=False, status=False)
    assert r["nodes"].tobytes() == full["nodes"].tobytes() and list(r) == ["nodes"]


# ---------------------------------------------------------------------------------- 7. scamd.rules and tools/perft.py
def test_rules_module_and_tool(scamd, fen, rules, orc, capsys):
    fens = [perft_ref.KIWI, perft_ref.POS4]
    raw = run(scamd, fen, [(f, []) for f in fens], 2)
    r = rules.perft([[], []], 2, fens=fens, divide=True, kinds=True)
    assert r["nodes"].dtype == np.uint64 and r["nodes"].tolist() == raw["nodes"].tolist() and not r["status"].any()
    for k, name in enumerate(rules.KINDS):
        assert r["kinds"][name].tolist() == raw["kinds"][:, 1 + k].tolist(), name
    for i in range(2):
        assert r["divide"][i] == [(scamd.move_uci(m), c) for m, c in _divide(raw, i)]
    assert set(rules.perft([[]], 2)) == {"nodes", "status"}
    lm = rules.legal_moves([[], []], fens=fens)
    assert lm == [orc.State(f).legal_uci() for f in fens]
    assert rules.legal_moves([["e2e4"]]) == [[orc.uci(m) for m in _after(orc, ["e2e4"]).legal_moves()]]
    with pytest.raises(ValueError, match="not legal"):
        rules.legal_moves([["e2e5"]])
    import perft as tool
    capsys.readouterr()
    tool.main(["--fen", perft_ref.KIWI, "--depth", "2", "--kinds"])
    text = capsys.readouterr().out
    rows = [ln.split(": ") for ln in text.split("\n\n")[0].splitlines()]
    assert [u for u, _ in rows] == orc.State(perft_ref.KIWI).legal_uci() and sum(int(c) for _, c in rows) == 2039
    assert "Nodes searched: 2039" in text and "castles: 91" in text


def _after(orc, moves):
    st = orc.State()
    for m in moves:
        st.push(m)
    return st
