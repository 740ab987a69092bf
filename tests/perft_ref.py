"""The yardstick of the perft tests: a plain Python walk over the CPU oracle's State (legal_moves, push / pop, is_check,
piece_at) that returns what sc_perft returns -- nodes, the six kinds of the last moves, the divide -- by the definitions of
include/sc_engine.h, and the expected values as constants.

TABLE was computed on the CPU with the oracle and this classifier.  Rows 1-4 agree with the Chess Programming Wiki's perft tables
in every column; the wiki has no kind counts for rows 5 and 6; rows 7 and 8 are the mate / stalemate probes and not from it."""

START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
KIWI = "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1"
POS3 = "8/2p5/3p4/KP5r/1R3p1k/8/4P1P1/8 w - - 0 1"
POS4 = "r3k2r/Pppp1ppp/1b3nbN/nP6/BBP1P3/q4N2/Pp1P2PP/R2Q1RK1 w kq - 0 1"
POS5 = "rnbq1k1r/pp1Pbppp/2p5/8/2B5/8/PPP1NnPP/RNBQK2R w KQ - 1 8"
POS6 = "r4rk1/1pp1qppp/p1np1n2/2b1p1B1/2B1P1b1/P1NP1N2/1PP1QPPP/R4RK1 w - - 0 10"
PAWN_ENDING = "8/8/8/8/8/5k2/4p3/4K3 b - - 0 1"        # one of Black's six moves stalemates White
QUEEN_MATE = "k7/8/K7/8/8/8/8/1Q6 w - - 0 1"             # one of White's 24 moves mates
WIDE = "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1"   # 218 legal moves, the known maximum

KINDS = ("captures", "ep", "castles", "promotions", "checks", "checkmates")

# fen -> {depth: (nodes, captures, ep, castles, promotions, checks, checkmates)}; None: the column is not in the table
TABLE = {
    START: {3: (8902, 34, 0, 0, 0, 12, 0), 4: (197281, 1576, 0, 0, 0, 469, 8), 5: (4865609, 82719, 258, 0, 0, 27351, 347)},
    KIWI: {1: (48, 8, 0, 2, 0, 0, 0), 2: (2039, 351, 1, 91, 0, 3, 0), 3: (97862, 17102, 45, 3162, 0, 993, 1),
           4: (4085603, 757163, 1929, 128013, 15172, 25523, 43)},
    POS3: {3: (2812, 209, 2, 0, 0, 267, 0), 4: (43238, 3348, 123, 0, 0, 1680, 17), 5: (674624, 52051, 1165, 0, 0, 52950, 0)},
    POS4: {2: (264, 87, 0, 6, 48, 10, 0), 3: (9467, 1021, 4, 0, 120, 38, 22), 4: (422333, 131393, 0, 7795, 60032, 15492, 5)},
    POS5: {1: (44, 6, 0, 1, 4, 0, 0), 3: (62379, 8517, 0, 1081, 5068, 1201, 44), 4: (2103487, 296153, 0, 0, 0, 158486, 240)},
    POS6: {3: (89890, 9470, 0, 0, 0, 1783, 0), 4: (3894594, 440388, 0, 0, 0, 68985, 0)},
    PAWN_ENDING: {1: (6, 0, 0, 0, 0, 0, 0), 2: (13, 5, None, None, None, None, None), 3: (115, 0, 0, 0, 32, 16, 0), 4: (680, 77, 0, 0, 0, 0, 0)},
    QUEEN_MATE: {1: (24, 0, 0, 0, 0, 4, 1), 2: (20, 1, 0, 0, 0, 0, 0), 3: (465, 0, 0, 0, 0, 102, 5)},
}
# published node totals beyond the table
DEEP = ((START, 6, 119060324), (KIWI, 5, 193690690), (POS3, 6, 11030083))
SMALL = 100000   # rows of at most about this many nodes are walked in Python too


def classify(st, m):
    """the kinds of move m (a legal move of st) as a 6-tuple of 0 / 1, st unchanged"""
    frm, to, promo = m & 63, (m >> 6) & 63, (m >> 12) & 7
    mover, target = abs(st.piece_at(frm)), st.piece_at(to)
    ep = mover == 1 and target == 0 and (frm & 7) != (to & 7)       # a pawn that changes file onto an empty square
    castle = mover == 6 and abs((frm & 7) - (to & 7)) == 2           # the king moves two files
    st.push(m)
    check = st.is_check()
    mate = check and not st.legal_moves()
    st.pop()
    return (int(target != 0 or ep), int(ep), int(castle), int(promo != 0), int(check), int(mate))


def walk(st, depth):
    """-> (nodes, [captures, ep, castles, promotions, checks, checkmates]) over the sequences of exactly `depth` legal moves"""
    if depth == 0:
        return 1, [0] * 6
    nodes, kinds = 0, [0] * 6
    for m in st.legal_moves():
        if depth == 1:
            nodes += 1
            for k, v in enumerate(classify(st, m)):
                kinds[k] += v
        else:
            st.push(m)
            n, kd = walk(st, depth - 1)
            st.pop()
            nodes += n
            for k in range(6):
                kinds[k] += kd[k]
    return nodes, kinds


def perft(st, depth):
    """sc_perft's outputs for one entry: dict(nodes, kinds=[6], divide=[(move, count), ...] in the oracle's order)"""
    if depth == 0:
        return dict(nodes=1, kinds=[0] * 6, divide=[])
    nodes, kinds, divide = 0, [0] * 6, []
    for m in st.legal_moves():
        if depth == 1:
            n, kd = 1, list(classify(st, m))
        else:
            st.push(m)
            n, kd = walk(st, depth - 1)
            st.pop()
        divide.append((m, n))
        nodes += n
        for k in range(6):
            kinds[k] += kd[k]
    return dict(nodes=nodes, kinds=kinds, divide=divide)


def divide_by_oracle(st, depth):
    """the divide from the oracle's own perft: push(m); perft(depth - 1)"""
    out = []
    for m in st.legal_moves():
        st.push(m)
        out.append((m, st.perft(depth - 1)))
        st.pop()
    return out
