"""Chess, the oracle and pure-Python data -- nothing here touches the package, the device or a process (tests/support.py does):
  san_to_move                                  SAN parsing on top of the oracle's legal-move list
  random_games, special_walk, random_steps     seeded games, and a game's steps with shuffled children and visit counts
  bits, golden_boards                          the float32 -> uint32 view, the four golden network inputs
  edge_features, line_features, EDGE_CATEGORIES, load_edge_lines      the edge-case predicates and their corpus
  _same_tree, assert_same_tree_bits, _assert_same, GpuPredictEvaluator   a device search tree against the oracle's
The named move lines and tables are tests/lines.py."""
import ctypes as C
import os
import random

import numpy as np

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")   # support.GOLD; tools import this module without pytest
PT ={"N": 2, "B": 3, "R": 4, "Q": 5, "K": 6}


def san_to_move(st, san, orc):
    """Resolve a SAN token against the oracle's legal moves; returns (move, gives_check_flag, mate_flag)."""
    s = san.strip()
    mate = s.endswith("#")
    check = s.endswith("+") or mate
    s = s.rstrip("+#")
    legal = st.legal_moves()
    turn = st.turn
    if s in ("O-O", "O-O-O"):
        base = 0 if turn else 56
        to = base + (6 if s == "O-O" else 2)
        cands = [m for m in legal if (m & 63) == base + 4 and ((m >> 6) & 63) == to and abs(st.piece_at(base + 4)) == 6]
        assert len(cands) == 1, (san, st.fen())
        return cands[0], check, mate
    promo = 0
    if "=" in s:
        s, pr = s.split("=")
        promo = PT[pr]
    piece = 1
    if s[0] in PT:
        piece = PT[s[0]]
        s = s[1:]
    s = s.replace("x", "")
    to = (ord(s[-1]) - 49) * 8 + (ord(s[-2]) - 97)
    dis = s[:-2]
    cands = []
    for m in legal:
        f, t, p = m & 63, (m >> 6) & 63, (m >> 12) & 7
        if t != to or p != promo or abs(st.piece_at(f)) != piece:
            continue
        ok = True
        for ch in dis:
            if ch in "abcdefgh" and (f & 7) != ord(ch) - 97:
                ok = False
            if ch in "12345678" and (f >> 3) != ord(ch) - 49:
                ok = False
        if ok:
            cands.append(m)
    assert len(cands) == 1, (san, st.fen(), [orc.uci(c) for c in cands])
    return cands[0], check, mate


def random_games(orc, n, maxlen, seed):
    """[(moves, State)] with a bias towards knight shuffles (repetitions) in every third game."""
    rnd = random.Random(seed)
    games = []
    for g in range(n):
        st = orc.State()
        mv = []
        for _ in range(rnd.randint(0, maxlen)):
            lm = st.legal_moves()
            if not lm:
                break
            if g % 3 == 0:
                pref = [x for x in lm if abs(st.piece_at(x & 63)) == 2]
                m = rnd.choice(pref) if pref and rnd.random() < 0.8 else rnd.choice(lm)
            else:
                m = rnd.choice(lm)
            st.push(m)
            mv.append(m)
        games.append((mv, st))
    return games


def random_steps(orc, moves, rnd, zero_share=0.0):
    """[(move, [(child, visits)])] of a game: every ply's legal moves in an order shuffled by `rnd`, visits drawn from 0..200.
    With zero_share > 0 a draw of rnd.random() comes first for every child and makes that share of the counts 0 (then without
    a randint); with zero_share == 0 no such draw is made, so the calls on `rnd` are those of the plain form"""
    st = orc.State()
    steps = []
    for m in moves:
        lm = st.legal_moves()
        order = list(range(len(lm)))
        rnd.shuffle(order)
        if zero_share:
            steps.append((m, [(lm[i], rnd.randint(0, 200) if rnd.random() < 1.0 - zero_share else 0) for i in order]))
        else:
            steps.append((m, [(lm[i], rnd.randint(0, 200)) for i in order]))
        st.push(m)
    return steps


def bits(a):
    """the bit patterns of float32 values: -0.0 is not +0.0, a NaN equals itself"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def golden_boards():
    return np.load(os.path.join(_GOLDEN, "nn_ref_b1_c256.npz"))["boards"][[0, 3, 5, 7]]


# ------------------------------------------------------------------ edge-case predicates (oracle primitives only)
# A move is from | to << 6 | promo << 12; piece_at gives +type for White, -type for Black (P=1 N=2 B=3 R=4 Q=5 K=6).
_KN = [(1, 2), (2, 1), (2, -1), (1, -2), (-1, -2), (-2, -1), (-2, 1), (-1, 2)]
_KG = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
_ORTH = [(1, 0), (0, 1), (-1, 0), (0, -1)]
_DIAG = [(1, 1), (-1, 1), (-1, -1), (1, -1)]


def mv_parts(m):
    return m & 63, (m >> 6) & 63, (m >> 12) & 7


def board_of(st):
    return [st.piece_at(sq) for sq in range(64)]


def _step(sq, df, dr):
    f, r = (sq & 7) + df, (sq >> 3) + dr
    return r * 8 + f if 0 <= f < 8 and 0 <= r < 8 else -1


def _ray(sq, df, dr):
    out = []
    s = _step(sq, df, dr)
    while s >= 0:
        out.append(s)
        s = _step(s, df, dr)
    return out


def attackers(b, sq, white):
    """squares of the pieces of colour `white` that attack sq on board b"""
    sg = 1 if white else -1
    out = []
    for df in (-1, 1):   # a pawn of that colour one rank behind sq
        s = _step(sq, df, -1 if white else 1)
        if s >= 0 and b[s] == sg:
            out.append(s)
    out += [s for s in (_step(sq, a, c) for a, c in _KN) if s >= 0 and b[s] == 2 * sg]
    out += [s for s in (_step(sq, a, c) for a, c in _KG) if s >= 0 and b[s] == 6 * sg]
    for dirs, kinds in ((_ORTH, (4, 5)), (_DIAG, (3, 5))):
        for df, dr in dirs:
            for s in _ray(sq, df, dr):
                if b[s]:
                    if b[s] * sg > 0 and abs(b[s]) in kinds:
                        out.append(s)
                    break
    return out


def _direction(a, b_):
    """unit (df, dr) from square a towards b_ if they share a rank, file or diagonal, else None"""
    df, dr = (b_ & 7) - (a & 7), (b_ >> 3) - (a >> 3)
    if a == b_ or not (df == 0 or dr == 0 or abs(df) == abs(dr)):
        return None
    return (df > 0) - (df < 0), (dr > 0) - (dr < 0)


def pin_line(b, sq):
    """the squares of the ray from the own king through the piece on sq if it is pinned (absolutely), else None"""
    if not b[sq]:
        return None
    sg = 1 if b[sq] > 0 else -1
    if 6 * sg not in b:
        return None
    k = b.index(6 * sg)
    d = _direction(k, sq)
    if d is None:
        return None
    ray = _ray(k, *d)
    i = ray.index(sq)
    if any(b[s] for s in ray[:i]):
        return None
    kinds = (4, 5) if 0 in d else (3, 5)
    for s in ray[i + 1:]:
        if b[s]:
            return ray if b[s] * sg < 0 and abs(b[s]) in kinds else None
    return None


def _material(b):
    return tuple(sorted(abs(p) for p in b if p > 0)), tuple(sorted(abs(p) for p in b if p < 0))


def _last_info(st, last):
    """(moved type, captured piece code, the square the pawn taken en passant stood on or -1, castling field before)"""
    if last is None:
        return None
    fr, to, _ = mv_parts(last)
    st.pop()
    try:
        moved, cap, cas = abs(st.piece_at(fr)), st.piece_at(to), st.fen().split()[2]
        epsq = -1
        if moved == 1 and (fr & 7) != (to & 7) and not cap:
            epsq = (fr & 56) | (to & 7)
            cap = st.piece_at(epsq)
    finally:
        st.push(last)
    return moved, cap, epsq, cas


def _rep_features(st, f):
    """repetition across a double push / across lost castling rights: walks the game back with pop() and forward again"""
    hist = []   # (board + turn, castling field, ep field) from the current position back to the start
    popped = []
    while True:
        fen = st.fen().split()
        hist.append((fen[0] + fen[1], fen[2], fen[3]))
        if st.ply == 0:
            break
        popped.append(st.pop())
    for m in reversed(popped):
        st.push(m)
    hist = hist[::-1]   # hist[i]: the position after i moves, reached by moves[i - 1]
    moves = popped[::-1]
    cur = hist[-1]
    same_board = [i for i, h in enumerate(hist) if h[0] == cur[0]]
    if len(same_board) < 3:
        return
    if len({hist[i][1] for i in same_board}) > 1 and not st.is_repetition(3):
        f.add("rep_castling_lost")
    same = [i for i in same_board if hist[i][1] == cur[1]]
    i0 = same[0]
    if i0 == 0 or len(same) < 3:
        return
    fr, to, _ = mv_parts(moves[i0 - 1])
    st2 = _replay(st, moves[:i0])
    if abs(st2.piece_at(to)) != 1 or abs(to - fr) != 16:
        return
    adj = [s for s in (_step(to, -1, 0), _step(to, 1, 0)) if s >= 0 and st2.piece_at(s) == -st2.piece_at(to)]
    ep_legal = hist[i0][2] != "-"
    if ep_legal:
        if not st.is_repetition(len(same)):
            f.add("rep_dp_legal_ep")
    elif not adj:
        if st.is_repetition(5):
            f.add("rep_dp_plain_5")
        elif st.is_repetition(3):
            f.add("rep_dp_plain_3")
    elif st.is_repetition(3):
        f.add("rep_dp_ep_pinned")


def _replay(st, moves):
    o = type(st)()
    for m in moves:
        o.push(m)
    return o


def edge_features(st, last=None, repetition=True):
    """the named edge-case properties of the position st (last: the move that led to it, or None)"""
    f = set()
    b = board_of(st)
    us = st.turn
    sg = 1 if us else -1
    legal = st.legal_moves()
    ls = set(legal)
    chk = st.is_check()
    oc = st.outcome()
    n = len(legal)
    king = b.index(6 * sg) if 6 * sg in b else -1
    oking = b.index(-6 * sg) if -6 * sg in b else -1
    checkers = attackers(b, king, not us) if king >= 0 else []
    li = _last_info(st, last)
    fen = st.fen().split()
    rights = fen[2]
    if n > 64:
        f.add("wide64")
    if n > 128:
        f.add("wide128")
    # ---- en passant
    if last is not None:
        lf, lt, _ = mv_parts(last)
        if abs(b[lt]) == 1 and abs(lt - lf) == 16:
            ep = (lf + lt) // 2
            caps = [s for s in (_step(lt, -1, 0), _step(lt, 1, 0)) if s >= 0 and b[s] == sg]
            legal_ep = [c for c in caps if (c | ep << 6) in ls]
            if legal_ep:
                f.add("ep_legal")
            if len(legal_ep) == 2:
                f.add("ep_two_capturers")
            for c in caps:
                pl = pin_line(b, c)
                if c in legal_ep:
                    if pl is not None and ep in pl:
                        f.add("ep_pinned_along_pin")
                elif not chk:
                    if king >= 0 and (king >> 3) == (c >> 3):
                        f.add("ep_pin_horizontal")
                    elif pl is not None and 0 not in _direction(king, c):
                        f.add("ep_pin_diagonal")
            if chk and legal_ep and lt in checkers:
                f.add("ep_evades_pawn_check")
            # the double push uncovered a check: the ep capture neither takes the checker nor blocks (a line through the
            # pushed pawn's start square meets its ep square only on the file, where the pawn itself blocks), so it is illegal
            if chk and caps and any(c != lt for c in checkers):
                f.add("ep_discovered_check")
    if li and li[2] >= 0 and oc and oc["termination"] == "Checkmate":
        f.add("ep_mate")
    # ---- castling
    base = 0 if us else 56
    ks, qs = (base + 4) | (base + 6) << 6, (base + 4) | (base + 2) << 6
    if ks in ls and qs in ls:
        f.add("castle_both")
    if qs in ls and attackers(b, base + 1, not us):
        f.add("castle_queenside_b_attacked")
    for ch, mv, path in (("K" if us else "k", ks, (base + 5, base + 6)), ("Q" if us else "q", qs, (base + 1, base + 2, base + 3))):
        if ch in rights and not any(b[s] for s in path):
            if chk:
                f.add("castle_in_check")
            elif mv not in ls:
                f.add("castle_path_attacked")
    if li:
        moved, cap, _, cas_before = li
        lf, lt, lp = mv_parts(last)
        if abs(cap) == 4 and lt in (0, 7, 56, 63) and cas_before != rights:
            f.add("rights_lost_rook_captured")
        if moved == 6 and abs(lt - lf) == 2 and chk:
            f.add("castle_gives_check")
        if lp == 2 and chk:
            f.add("underpromo_knight_check")
    for white, kch, qch in ((True, "K", "Q"), (False, "k", "q")):
        s = 1 if white else -1
        hb = 0 if white else 56
        if b[hb + 4] == 6 * s:
            for c, other, corner in ((kch, qch, hb + 7), (qch, kch, hb)):
                if b[corner] == 4 * s and c not in rights and other in rights:
                    f.add("rights_lost_rook_returned")
    # ---- promotion
    promos = [m for m in legal if m >> 12]
    for m in promos:
        fr, to, p = mv_parts(m)
        if p == 5 and (fr & 7) == (to & 7) and all((fr | to << 6 | q << 12) in ls for q in (2, 3, 4)):
            f.add("promo_push_all_four")
        if p == 5 and (fr & 7) - (to & 7) == 1 and (fr | (to + 2) << 6 | 5 << 12) in ls:
            f.add("promo_capture_both_sides")
        pl = pin_line(b, fr)
        if pl is not None and to in pl:
            f.add("promo_pinned_along_pin")
        if chk and to in checkers:
            f.add("promo_captures_checker")
    # ---- checks and pins
    if len(checkers) >= 2:
        f.add("double_check")
        if any((king | c << 6) in ls for c in checkers):
            f.add("double_check_king_takes")
    for c in checkers:
        if abs(b[c]) in (3, 4, 5):
            d = _direction(c, king)
            t = _step(king, *d)
            if t >= 0 and b[t] * sg <= 0 and (king | t << 6) not in ls:
                b2 = list(b)
                b2[king] = 0
                if c in attackers(b2, t, not us):
                    f.add("king_xray_step")
    for sq in range(64):
        if b[sq] * sg in (2, 3, 4, 5) and pin_line(b, sq) is not None:
            if b[sq] * sg == 2:
                f.add("pinned_knight")
            elif any((m & 63) == sq for m in legal):
                f.add("pinned_slider_moves")
    if king >= 0 and oking >= 0:
        df, dr = abs((king & 7) - (oking & 7)), abs((king >> 3) - (oking >> 3))
        if sorted((df, dr)) == [0, 2]:
            f.add("kings_opposition")
    # ---- terminations
    if oc:
        f.add({"Checkmate": "checkmate", "Stalemate": "stalemate", "FiftyMoves": "fifty_moves", "SeventyfiveMoves": "seventyfive_moves",
               "ThreefoldRepetition": "threefold", "FivefoldRepetition": "fivefold"}.get(oc["termination"], "insufficient"))
    mat = _material(b)
    bishops = [sq for sq in range(64) if abs(b[sq]) == 3]
    colours = {((s & 7) + (s >> 3)) & 1 for s in bishops}
    insuf = bool(oc) and oc["termination"] == "InsufficientMaterial"
    kinds = {((6,), (6,)): "KvK", ((2, 6), (6,)): "KNvK", ((6,), (2, 6)): "KNvK", ((3, 6), (6,)): "KBvK", ((6,), (3, 6)): "KBvK"}
    if insuf and mat in kinds:
        f.add("insufficient_" + kinds[mat])
    if mat == ((3, 6), (3, 6)):
        f.add("insufficient_KBvKB_same" if insuf and len(colours) == 1 else "near_KBvKB_opposite" if not insuf and len(colours) == 2 else "?")
    if mat in (((2, 2, 6), (6,)), ((6,), (2, 2, 6))) and not insuf:
        f.add("near_KNNvK")
    f.discard("?")
    f.discard("insufficient")
    if repetition and (st.is_repetition(2) or "fifty_moves" in f or oc):
        _rep_features(st, f)
    return f


def special_walk(orc, n, maxlen, seed, starts=None):
    """[(moves, State)] random games that play an en-passant capture, a castling move, a promotion, a check or a double push
    next to an enemy pawn whenever one is legal (in that order of preference, each with high probability); game g opens with
    the moves starts[g % len(starts)] if starts are given"""
    rnd = random.Random(seed)
    games = []
    for g in range(n):
        st = orc.State()
        mv = []
        for m in (starts[g % len(starts)] if starts else []):
            st.push(m)
            mv.append(m)
        for _ in range(rnd.randint(maxlen // 2, maxlen)):
            lm = st.legal_moves()
            if not lm or st.outcome():
                break
            b = board_of(st)
            ep, cas, pro, dbl = [], [], [], []
            for m in lm:
                fr, to, p = mv_parts(m)
                if abs(b[fr]) == 1 and (fr & 7) != (to & 7) and not b[to]:
                    ep.append(m)
                elif abs(b[fr]) == 6 and abs(to - fr) == 2:
                    cas.append(m)
                elif p:
                    pro.append(m)
                elif abs(b[fr]) == 1 and abs(to - fr) == 16 and any(
                        s >= 0 and b[s] == -b[fr] for s in (_step(to, -1, 0), _step(to, 1, 0))):
                    dbl.append(m)
            m = None
            for group, prob in ((ep, 0.9), (cas, 0.25), (pro, 0.8), (dbl, 0.6)):
                if group and rnd.random() < prob:
                    m = rnd.choice(group)
                    break
            if m is None and rnd.random() < 0.3:
                checks = []
                for x in lm:
                    st.push(x)
                    if st.is_check():
                        checks.append(x)
                    st.pop()
                if checks:
                    m = rnd.choice(checks)
            if m is None:
                m = rnd.choice(lm)
            st.push(m)
            mv.append(m)
        games.append((mv, st))
    return games


# every category of tests/golden/edge_lines.json and the number of distinct lines it must hold (tools/find_edge_lines.py)
EDGE_CATEGORIES = {c: 2 for c in (
    "ep_legal ep_pin_horizontal ep_pin_diagonal ep_pinned_along_pin ep_evades_pawn_check ep_discovered_check ep_two_capturers "
    "ep_mate castle_both castle_path_attacked castle_queenside_b_attacked castle_in_check rights_lost_rook_captured "
    "rights_lost_rook_returned castle_gives_check promo_push_all_four promo_capture_both_sides promo_pinned_along_pin "
    "promo_captures_checker underpromo_knight_check double_check double_check_king_takes king_xray_step pinned_knight "
    "pinned_slider_moves kings_opposition wide64 wide128 rep_dp_plain_3 rep_dp_plain_5 rep_dp_ep_pinned rep_dp_legal_ep "
    "rep_castling_lost checkmate stalemate insufficient_KvK insufficient_KNvK insufficient_KBvK insufficient_KBvKB_same "
    "near_KBvKB_opposite near_KNNvK fifty_moves seventyfive_moves threefold fivefold").split()}


def line_features(orc, uci):
    """edge_features of the final position of a UCI line from the start position"""
    st = orc.State()
    m = None
    for u in uci:
        m = orc.from_uci(u)
        st.push(m)
    return edge_features(st, m)


def load_edge_lines():
    import json
    with open(os.path.join(_GOLDEN, "edge_lines.json")) as fh:
        return json.load(fh)


# ------------------------------------------------------------------ device search tree against the oracle's
def _same_tree(t, d):
    """SelfPlay.tree(slot) equals Search.dump(): node count, N, value sums, uct words, moves, child counts"""
    return (len(t["n"]) == len(d["n"]) and np.array_equal(t["n"], d["n"]) and np.array_equal(t["q"], d["q"])
            and np.array_equal(t["uct"], d["uct"]) and np.array_equal(t["move"][1:], d["move"][1:])
            and np.array_equal(t["n_child"], d["n_child"]))


def assert_same_tree_bits(t, d, where):
    """_same_tree on the bit patterns (-0.0 is not +0.0, a NaN equals itself), naming the first node that differs"""
    assert len(t["n"]) == len(d["n"]), (where, "nodes", len(t["n"]), len(d["n"]))
    for k in ("n", "q", "uct", "n_child"):
        a, b = t[k].view(np.uint32), d[k].view(np.uint32)
        assert np.array_equal(a, b), (where, k, np.flatnonzero(a != b)[:8])
    assert np.array_equal(t["move"][1:], d["move"][1:]), (where, "move")
    assert _same_tree(t, d), where


class GpuPredictEvaluator:
    """orc_eval_fn (oracle/sc_oracle_mcts.h) that answers with the ENGINE's `predict` on the oracle's own encoding of the
    state: the post-_encode contract of src/backends/torch.rs:108-146."""

    def __init__(self, orc, eng):
        self.orc, self.eng, self.L = orc, eng, orc.lib()
        self.priors = []          # one array per expansion, in allocation order of the children
        self.values = []
        self.fn = orc.EVAL_FN(self._call)

    def _call(self, user, st, n_legal, legal, legal_idx, priors, value):
        boards = np.zeros((8, 8, 112), np.int8)
        meta = np.zeros(7, np.int32)
        self.L.orc_encode(st, boards.ctypes.data_as(C.c_void_p), meta.ctypes.data_as(C.c_void_p))
        idx = np.asarray([legal_idx[i] for i in range(n_legal)], np.uint16)
        pri, val = self.eng.predict(boards[None], meta[None], [idx])
        p = np.asarray(pri[0], np.float32)
        for i in range(n_legal):
            priors[i] = float(p[i])
        value[0] = float(val[0])
        self.priors.append(p.copy())
        self.values.append(np.float32(val[0]))


def _assert_same(t, d, ev, where):
    """the tree of a search fed by the network against the oracle's tree fed by `ev`, bit for bit, priors included"""
    n = len(d["n"])
    assert len(t["n"]) == n, where
    for k in ("n", "q", "uct", "n_child"):
        assert np.array_equal(t[k].view(np.uint32), d[k].view(np.uint32)), (where, k, np.flatnonzero(t[k] != d[k])[:8])
    assert np.array_equal(t["move"][1:], d["move"][1:]), where
    pri = np.concatenate(ev.priors) if ev.priors else np.zeros(0, np.float32)
    assert len(pri) == n - 1 and np.array_equal(t["prior"][1:].view(np.uint32), pri.view(np.uint32)), (where, "prior")
