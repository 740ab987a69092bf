"""The yardstick of the SAN tests, on the CPU oracle alone (it never calls the device): one renderer of a legal move as a SAN
word -- python-chess's Board.san() (Board._algebraic_without_suffix + the check marks) and two looser spellings the parser must
also read -- and the games, moves and one-hot steps built on it.  tests/test_san_ref.py checks this module against the words of
the reference's own games and against helpers.san_to_move."""
from collections import Counter

import helpers as H

_LET = {2: "N", 3: "B", 4: "R", 5: "Q", 6: "K"}

# the edge corpus has no short form that is unique only through a pin: after 3...d6 the knight on c6 is pinned, so 4...Ne7 is the g8 knight's
PINNED_RIVAL = ["e2e4", "e7e5", "g1f3", "b8c6", "f1b5", "d7d6", "e1g1", "g8e7"]


def _sq(s):
    return "abcdefgh"[s & 7] + str((s >> 3) + 1)


def san_of(st, m, style="min", seen=None):
    """SAN of the move m, which must be legal in oracle state st.  style "min": Board.san() -- no rival, nothing; a rival on the
    origin's rank (or on neither its rank nor its file), the file letter; a rival on the origin's file, the rank digit; pawns are
    never disambiguated; "=" before a promotion piece.  "noeq": the same without the "=".  "over": piece, origin square, "-" or
    "x", destination (castling with the digit 0).  seen counts the special cases rendered."""
    seen = Counter() if seen is None else seen
    legal = st.legal_moves()
    assert m in legal, (st.fen(), m)
    fr, to, pr = H.mv_parts(m)
    b = H.board_of(st)
    pt, white = abs(b[fr]), b[fr] > 0
    ep = pt == 1 and (fr & 7) != (to & 7) and not b[to]
    cap = bool(b[to]) or ep
    st.push(m)
    chk = st.is_check()
    suf = ("+" if st.legal_moves() else "#") if chk else ""
    st.pop()
    seen["ep"] += ep
    seen["promo_capture_check"] += bool(pr and cap and chk)
    seen["underpromo"] += pr in (2, 3, 4)
    if pt == 6 and abs(to - fr) == 2:
        seen["castle_k" if to > fr else "castle_q"] += 1
        s = "O-O" if to > fr else "O-O-O"
        return (s.replace("O", "0") if style == "over" else s) + suf
    promo = ("" if style == "noeq" else "=") + _LET[pr] if pr else ""
    if style == "over":
        return (_LET[pt] if pt > 1 else "") + _sq(fr) + ("x" if cap else "-") + _sq(to) + promo + suf
    if pt == 1:
        return ("abcdefgh"[fr & 7] + "x" if cap else "") + _sq(to) + promo + suf
    others = [x & 63 for x in legal if (x >> 6) & 63 == to and (x & 63) != fr and abs(b[x & 63]) == pt]
    dis = ""
    if others:
        row = any(o >> 3 == fr >> 3 for o in others)
        col = any(o & 7 == fr & 7 for o in others)
        dis = ("abcdefgh"[fr & 7] if row or not col else "") + (str((fr >> 3) + 1) if col else "")
        seen["file_dis" if not col else "file_and_rank" if row else "rank_dis"] += 1
    elif not st.is_check():
        # a rival of the same kind attacks the square too but is pinned off it: only legality makes the short form unique
        for r in H.attackers(b, to, white):
            pl = H.pin_line(b, r) if r != fr and abs(b[r]) == pt else None
            seen["pinned_rival"] += pl is not None and to not in pl
    return _LET[pt] + dis + ("x" if cap else "") + _sq(to) + promo + suf


def cpu_game(orc, moves, fen=None, seen=None, style="min"):
    """the words of a game from the start position, or from `fen`"""
    st = orc.State(fen) if fen else orc.State()
    words = []
    for m in moves:
        words.append(san_of(st, m, style, seen))
        st.push(m)
    return words


def yardstick_moves(orc, movetext):
    """helpers.san_to_move over the oracle, on the SAN words of a plain movetext (numbers and the result dropped here)"""
    st = orc.State()
    moves = []
    for w in movetext.split():
        if w[0].isdigit() and w not in ("0-0", "0-0-0") or w == "*":
            continue
        m, _, _ = H.san_to_move(st, w.replace("0", "O") if w.startswith("0-0") else w, orc)
        st.push(m)
        moves.append(m)
    return moves


def one_hot_steps(orc, moves):
    """ValidationDataset._to_trace: the children of a ply are the legal moves, count 1 on the move played"""
    st = orc.State()
    steps = []
    for m in moves:
        steps.append((m, [(x, 1 if x == m else 0) for x in st.legal_moves()]))
        st.push(m)
    return steps
