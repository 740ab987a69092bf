"""Writes tests/golden/edge_lines.json: short legal lines from the start position to positions with a named edge-case
property (en passant under pins and checks, castling rights and paths, promotions, double checks, repetitions across double
pushes and lost castling rights, every termination).  The properties are tests/helpers.py:edge_features, computed on the CPU
oracle; each category of helpers.EDGE_CATEGORIES gets its minimum number of distinct lines.

Lines come from hand-written sequences (HAND, below, for what a random search reaches too slowly), from random walks that
prefer special moves (helpers.special_walk), from capture walks that keep a chosen material set (insufficient material), and
from quiet piece walks (the 50 / 75 move rules).  Test tooling only; deterministic for a given seed:

    python tools/find_edge_lines.py [--seed 1] [--out tests/golden/edge_lines.json]
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle import oracle_py as orc  # noqa: E402
import helpers as H  # noqa: E402

# (name, category, line, note)
HAND = [
    ("ep_pin_rank_e5d6", "ep_pin_horizontal",
     "e2e4 a7a5 e4e5 a8a6 e1e2 a6h6 e2e3 h6h5 e3d4 g8f6 d4c4 f6g8 c4b5 d7d5",
     "e5xd6 is pseudo-legal but illegal: it clears b5-h5 and the rook on h5 would take the king"),
    ("ep_pin_rank_e5f6", "ep_pin_horizontal",
     "e2e4 a7a5 e4e5 a8a6 e1e2 a6h6 e2e3 h6h5 e3d4 g8f6 d4c4 f6g8 c4b5 f7f5",
     "e5xf6 is illegal for the same reason, the captured pawn on the king's far side"),
    ("ep_along_pin_queen", "ep_pinned_along_pin",
     "e2e4 c7c6 e4e5 d8c7 e1e2 a7a6 e2f3 a6a5 f3g3 d7d5",
     "the e5 pawn is pinned on g3-c7 by the queen; e5xd6 stays on the pin line and is legal"),
    ("ep_along_pin_bishop", "ep_pinned_along_pin",
     "e2e4 g7g6 e4e5 f8g7 e1e2 a7a6 e2e3 a6a5 e3d4 f7f5",
     "the e5 pawn is pinned on d4-g7 by the bishop; e5xf6 stays on the pin line and is legal"),
    ("ep_discovered_g4", "ep_discovered_check",
     "e2e4 a7a6 e4e5 a6a5 e1e2 a5a4 e2f3 a4a3 f3g4 d7d5",
     "d7-d5 uncovers the c8 bishop's check on g4: e5xd6 neither captures the checker nor blocks, so it is illegal"),
    ("ep_discovered_h3", "ep_discovered_check",
     "e2e4 a7a6 e4e5 a6a5 e1e2 a5a4 e2f3 a4a3 f3g3 h7h6 g3h3 d7d5",
     "the same on h3: the only evasions are king moves and interpositions"),
    ("ep_mate_d6", "ep_mate",
     "e2e4 e7e6 e4e5 e8e7 f1b5 c7c5 d1f3 d8a5 f3g3 b8c6 g1f3 c6d8 b1c3 g8f6 a2a3 d7d5 e5d6",
     "e5xd6 mates: the pawn checks e7, b5 covers d7 and e8, g3 guards d6 through the emptied e5, own pieces fill the rest"),
    ("ep_mate_d6_b", "ep_mate",
     "e2e4 e7e6 e4e5 e8e7 f1b5 c7c5 d1f3 d8a5 f3g3 b8c6 h2h3 c6d8 g1e2 g8f6 h3h4 d7d5 e5d6",
     "the same mate after other waiting moves"),
    ("castle_long_check", "castle_gives_check",
     "d2d4 e7e5 d4e5 d7d5 e2e4 d5e4 d1h5 e8d7 c1f4 a7a6 b1c3 a6a5 e1c1",
     "O-O-O puts the rook on d1 against the king on d7 down the emptied d-file"),
    ("rep_dp_plain_e4", "rep_dp_plain_3",
     "e2e4 g8f6 g1f3 f6g8 f3g1 g8f6 g1f3 f6g8 f3g1",
     "the position after e2-e4 (no black pawn next to e4: no ep in its identity) occurs a third time"),
    ("rep_dp_plain_d4", "rep_dp_plain_3",
     "d2d4 b8c6 b1c3 c6b8 c3b1 b8c6 b1c3 c6b8 c3b1",
     "the position after d2-d4 occurs a third time"),
    ("rep_dp_plain_e4_five", "rep_dp_plain_5",
     "e2e4 g8f6 g1f3 f6g8 f3g1 g8f6 g1f3 f6g8 f3g1 g8f6 g1f3 f6g8 f3g1 g8f6 g1f3 f6g8 f3g1",
     "the position after e2-e4 occurs a fifth time: FivefoldRepetition"),
    ("rep_dp_plain_c5_five", "rep_dp_plain_5",
     "g1f3 c7c5 b1c3 b8c6 c3b1 c6b8 b1c3 b8c6 c3b1 c6b8 b1c3 b8c6 c3b1 c6b8 b1c3 b8c6 c3b1 c6b8",
     "the position after c7-c5 occurs a fifth time"),
    ("rep_dp_pinned_d5", "rep_dp_ep_pinned",
     "e2e4 a7a5 e4e5 a8a6 e1e2 a6h6 e2e3 h6h5 e3d4 g8f6 d4c4 f6g8 c4b5 d7d5 g1f3 g8f6 f3g1 f6g8 g1f3 g8f6 f3g1 f6g8",
     "after d7-d5 the only ep capture is pinned (illegal): the position repeats with it three times"),
    ("rep_dp_pinned_f5", "rep_dp_ep_pinned",
     "e2e4 a7a5 e4e5 a8a6 e1e2 a6h6 e2e3 h6h5 e3d4 g8f6 d4c4 f6g8 c4b5 f7f5 b1c3 b8c6 c3b1 c6b8 b1c3 b8c6 c3b1 c6b8",
     "after f7-f5 the only ep capture is pinned (illegal): the position repeats with it three times"),
    ("rep_dp_legal_ep_d5", "rep_dp_legal_ep",
     "e2e4 a7a6 e4e5 d7d5 g1f3 g8f6 f3g1 f6g8 g1f3 g8f6 f3g1 f6g8",
     "the board after d7-d5 recurs twice, but there e5xd6 was legal: it is a different position (no threefold)"),
    ("rep_dp_legal_ep_e5", "rep_dp_legal_ep",
     "d2d4 h7h6 d4d5 e7e5 b1c3 b8c6 c3b1 c6b8 b1c3 b8c6 c3b1 c6b8",
     "the board after e7-e5 recurs twice, but there d5xe6 was legal"),
    ("rep_castling_king", "rep_castling_lost",
     "e2e4 e7e5 e1e2 e8e7 e2e1 e7e8 e1e2 e8e7 e2e1 e7e8",
     "the board after e7-e5 recurs twice without castling rights: no threefold"),
    ("rep_castling_rook", "rep_castling_lost",
     "g1f3 g8f6 h1g1 h8g8 g1h1 g8h8 h1g1 h8g8 g1h1 g8h8",
     "the rooks go out and back: the board recurs twice without the kingside rights"),
    ("threefold_knights", "threefold",
     "e2e4 e7e5 g1f3 b8c6 f3g1 c6b8 g1f3 b8c6 f3g1 c6b8",
     "claimable threefold repetition"),
    ("threefold_bishops", "threefold",
     "e2e4 e7e5 f1c4 f8c5 c4f1 c5f8 f1c4 f8c5 c4f1 c5f8",
     "claimable threefold repetition"),
    ("fivefold_start", "fivefold", "g1f3 g8f6 f3g1 f6g8 " * 4, "the start position a fifth time"),
    ("fivefold_queenside", "fivefold", "b1c3 b8c6 c3b1 c6b8 " * 3 + "b1a3 b8a6 a3b1 a6b8", "the start position a fifth time"),
]


def _uci(moves):
    return [orc.uci(m) for m in moves]


def _walk_lines(games):
    """{category: [line, ...]} every ply of every game, each category's lines shortest first (ties: game order)"""
    found = {}
    for moves, _ in games:
        st = orc.State()
        for i, m in enumerate(moves):
            st.push(m)
            for f in H.edge_features(st, m, repetition=False):
                found.setdefault(f, []).append(moves[:i + 1])
    for f in found:
        found[f].sort(key=len)
    return found


def _material_walk(rnd, keep, maxlen=400):
    """capture-preferring walk that never removes a piece on a square in `keep` (the starting squares of the pieces to keep) and
    promotes to queens only; ends at the first position with exactly the kept pieces, or None"""
    st = orc.State()
    moves = []
    alive = set(keep)   # squares the kept pieces stand on now
    for _ in range(maxlen):
        lm = st.legal_moves()
        if not lm:
            return None
        b = H.board_of(st)
        ok = []
        for m in lm:
            fr, to, p = H.mv_parts(m)
            if to in alive or (p and p != 5):
                continue
            ok.append(m)
        caps = [m for m in ok if b[(m >> 6) & 63] or (abs(b[m & 63]) == 1 and (m & 7) != ((m >> 6) & 7))]
        pool = caps if caps and rnd.random() < 0.9 else ok
        if not pool:
            return None
        m = rnd.choice(pool)
        fr, to, _ = H.mv_parts(m)
        if fr in alive:
            alive.discard(fr)
            alive.add(to)
        st.push(m)
        moves.append(m)
        if sum(1 for x in H.board_of(st) if x) == len(alive) + 2:
            return moves
        if st.outcome():
            return None
    return None


def _quiet_walk(rnd, target, maxlen=400):
    """a few random opening plies, then random quiet piece moves (no capture, no pawn move) that end nothing early, until the
    outcome is `target` (FiftyMoves / SeventyfiveMoves)"""
    st = orc.State()
    moves = []
    for i in range(maxlen):
        lm = st.legal_moves()
        b = H.board_of(st)
        if i < 8:
            pool = [m for m in lm if abs(b[m & 63]) == 1]
        else:
            pool = [m for m in lm if abs(b[m & 63]) != 1 and not b[(m >> 6) & 63]]
        rnd.shuffle(pool)
        for m in pool:
            st.push(m)
            oc = st.outcome()
            if oc is None or oc["termination"] in (target, "FiftyMoves"):
                break
            st.pop()
        else:
            return None
        moves.append(m)
        if oc and oc["termination"] == target:
            return moves
    return None


def generate(seed):
    rnd = random.Random(seed)
    lines = []
    have = {}

    def add(name, cat, uci, note):
        feats = H.line_features(orc, uci)
        assert cat in feats, (name, cat, sorted(feats))
        if any(e["uci"] == uci for e in lines):
            return False
        lines.append({"name": name, "category": cat, "uci": list(uci), "note": note})
        have[cat] = have.get(cat, 0) + 1
        return True

    for name, cat, line, note in HAND:
        add(name, cat, line.split(), note)
    from lines import WIDE, WIDE137
    add("wide82", "wide64", WIDE, "82 legal moves (tests/lines.py WIDE)")
    add("wide137", "wide128", WIDE137, "137 legal moves, seven white queens (tests/lines.py WIDE137)")
    # a second >128 position: WIDE137 plus one quiet pair of moves that keeps White's count above 128
    st = orc.State()
    for u in WIDE137:
        st.push(u)
    for w in st.legal_moves():
        st.push(w)
        done = False
        for bl in st.legal_moves():
            st.push(bl)
            if len(st.legal_moves()) > 128 and st.outcome() is None:
                done = add("wide137_plus2", "wide128", WIDE137 + _uci([w, bl]), "WIDE137 and one more move each, still > 128")
            st.pop()
            if done:
                break
        st.pop()
        if done:
            break
    # random walks that prefer special moves, in batches of 500 games until no walk finds anything new
    for batch in range(6):
        found = _walk_lines(H.special_walk(orc, 500, 200, seed * 1000 + batch))
        for cat in H.EDGE_CATEGORIES:
            for mv in found.get(cat, []):
                if have.get(cat, 0) >= H.EDGE_CATEGORIES[cat]:
                    break
                add(f"{cat}_walk{have.get(cat, 0)}", cat, _uci(mv), "special-move random walk")
        if all(have.get(c, 0) >= n for c, n in H.EDGE_CATEGORIES.items() if not c.startswith(("insufficient", "near", "fifty", "seventy"))):
            break
    # material walks: keep the named pieces (start squares), capture everything else
    keeps = [("insufficient_KvK", ()), ("insufficient_KNvK", (1,)), ("insufficient_KNvK", (62,)), ("insufficient_KBvK", (5,)),
             ("insufficient_KBvK", (58,)), ("insufficient_KBvKB_same", (5, 58)), ("near_KBvKB_opposite", (5, 61)),
             ("near_KBvKB_opposite", (2, 58)), ("near_KNNvK", (1, 6)), ("near_KNNvK", (57, 62)),
             ("insufficient_KvK", ()), ("insufficient_KBvKB_same", (2, 61))]
    for cat, keep in keeps:
        for _ in range(4000):
            if have.get(cat, 0) >= 2:
                break
            mv = _material_walk(rnd, keep)
            if mv and cat in H.line_features(orc, _uci(mv)):
                add(f"{cat}_{have.get(cat, 0)}", cat, _uci(mv), "capture walk keeping " + (" ".join(orc.uci(k | k << 6)[:2] for k in keep) or "nothing"))
                break
    for cat, target in (("fifty_moves", "FiftyMoves"), ("seventyfive_moves", "SeventyfiveMoves")):
        for _ in range(100):
            if have.get(cat, 0) >= 2:
                break
            mv = _quiet_walk(rnd, target)
            if mv:
                add(f"{cat}_{have.get(cat, 0)}", cat, _uci(mv), "quiet piece moves only after eight pawn moves")
    missing = {c: have.get(c, 0) for c, n in H.EDGE_CATEGORIES.items() if have.get(c, 0) < n}
    return lines, missing


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "edge_lines.json"))
    a = ap.parse_args()
    lines, missing = generate(a.seed)
    if missing:
        sys.exit(f"categories short of lines: {missing}")
    with open(a.out, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(e) for e in lines) + "\n]\n")
    print(f"{len(lines)} lines, {sum(len(e['uci']) for e in lines)} plies -> {a.out}")


if __name__ == "__main__":
    main()
