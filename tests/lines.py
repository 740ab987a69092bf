"""Named move lines and tables the tests and tools share: plain data, and the one function that plays a line on the oracle.
No test file defines these again, and nothing imports them from a test file."""

# 18 plies from the start position to a White-to-move position with 82 legal moves (found by a beam search on the
# oracle's move generator, tools/find_wide_position.py): the root of a search from here has more than 64 children
WIDE = ("e2e3 d7d5 d1g4 d8d6 f1b5 e8d8 b1c3 d6h2 c3d5 h2d6 h1h6 d6a3 b2b3 a3a4 c1b2 c7c5 b2e5 a4b3").split()
# 112 plies to a White-to-move position with 137 legal moves (seven white queens; found by a promotion-driven greedy search on
# the oracle's move generator): a root with more than 128 children -- the third round of lanes of the descent's wide level
WIDE137 = ("h2h4 g8h6 a2a4 h6g4 f2f4 g4h6 a4a5 h6g4 d2d4 g4f2 e1f2 b8a6 h4h5 a6b4 c2c4 b4c2 "
           "d1c2 d7d5 c4c5 e8d7 f4f5 d7e8 c2a4 b7b5 a5b6 c7c6 a4c6 c8d7 c6d5 f7f6 b6b7 d8c8 "
           "c5c6 e8d8 d5a5 d8e8 c6d7 e8f7 a5a2 c8c4 a2c4 e7e6 b7a8q f7g8 d7d8q g8f7 f5e6 f7g8 "
           "g2g4 a7a5 d4d5 g7g6 h5h6 f6f5 g4g5 a5a4 e6e7 g8f7 e7e8q f7g8 b2b4 f5f4 e2e4 f4f3 "
           "e4e5 a4a3 e5e6 a3a2 e6e7 a2b1q a1a6 b1f5 d5d6 f5f7 d6d7 f7d5 a6g6 h7g6 e7f8q g8h7 "
           "d8e7 d5f7 d7d8q h8g8 e8f7 h7h8 h6h7 g8f8 b4b5 f8g8 b5b6 g8e8 b6b7 e8g8 b7b8q g8e8 "
           "h1h2 e8g8 c4c2 g8e8 e7e4 e8g8 a8a3 g8e8 f7e8 h8g7 f2g3 f3f2 e8e5 g7f7 h7h8q f2g1b").split()
# five roots for the tests that put the network inside the search, and the slots of a 64-slot handle they are set in
LINES = [
    [],                                                        # start position: history planes empty
    ["e2e4", "c7c5", "g1f3"],                                  # Black to move: rotated view, short history
    ["f2f3", "e7e5", "g2g4"],                                  # mate in one among the children: terminal leaves
    WIDE,                                                      # 82 legal moves (two rounds of lanes), full 8-board history
    ["g1f3", "g8f6", "f3g1", "f6g8", "g1f3", "g8f6", "f3g1"],  # repetition planes set, Black to move
]
SLOTS = [0, 17, 31, 40, 63]
MATED = ["f2f3", "e7e5", "g2g4", "d8h4"]   # White is checkmated: a game set to this line ends after its first search

# public perft known answers: FEN -> node counts at depth 1, 2, ...
PERFT = {
    "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1": [20, 400, 8902, 197281],
    "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1": [48, 2039, 97862],
    "8/2p5/3p4/KP5r/1R3p1k/8/4P1P1/8 w - - 0 1": [14, 191, 2812, 43238],
    "r3k2r/Pppp1ppp/1b3nbN/nP6/BBP1P3/q4N2/Pp1P2PP/R2Q1RK1 w kq - 0 1": [6, 264, 9467],
    "rnbq1k1r/pp1Pbppp/2p5/8/2B5/8/PPP1NnPP/RNBQK2R w KQ - 1 8": [44, 1486, 62379],
    "r4rk1/1pp1qppp/p1np1n2/2b1p1B1/2B1P1b1/P1NP1N2/1PP1QPPP/R4RK1 w - - 0 10": [46, 2079, 89890],
}


def pushed(orc, moves):
    """the oracle's State after `moves` from the start position"""
    st = orc.State()
    for m in moves:
        st.push(m)
    return st
