"""Games written as SAN movetext (PGN files, the reference's py/validation/sample.csv) -> moves and training tensors on the GPU
(csrc/san_tokens.cpp, csrc/san_kernels.hip, sc_encode_san_device): the reference's ValidationDataset (py/dataset.py:90-128)
without python-chess.  The rules exist on the GPU only, so SAN is resolved there, against the generated legal moves.
The other direction too: moves -> SAN on the GPU (csrc/san_write_kernels.hip, sc_moves_to_san_device), movetext and PGN files."""
import csv
import ctypes as C
import re

import numpy as np

from .binding import _check, _count, _moves, _p, _stream, _torch, _tp, lib
from .training import _device_outputs, _finish_outputs

TOKEN_RESERVED = np.uint64(0xFFFFFFFFFFFFFFFF)
ERR_CAPACITY = -4   # SC_ERR_CAPACITY
_WINNER = {"white": 1.0, "black": -1.0, "draw": 0.0, None: 0.0, "": 0.0}
_RESULT = {"1-0": "white", "0-1": "black", "1/2-1/2": "draw"}


def tokenize(text):
    """One game's movetext -> uint64 array, one token per half-move (sc_san_tokenize; no GPU needed): the SAN characters,
    first character in the lowest byte, without check / annotation suffixes; 0xFFFFFFFFFFFFFFFF where a half-move does not fit."""
    L = lib()
    raw = text.encode() if isinstance(text, str) else bytes(text)
    n = C.c_uint32(0)
    out = np.zeros(len(raw) // 3 + 8, np.uint64)
    rc = L.sc_san_tokenize(raw, len(raw), _p(out), out.size, C.byref(n))
    if rc == ERR_CAPACITY:
        out = np.zeros(n.value, np.uint64)
        rc = L.sc_san_tokenize(raw, len(raw), _p(out), out.size, C.byref(n))
    _check(rc)
    return out[:n.value].copy()


def token_text(tok):
    """the characters of a token (for messages)"""
    return "<reserved>" if int(tok) == int(TOKEN_RESERVED) else int(tok).to_bytes(8, "little").rstrip(b"\0").decode("latin-1")


def pack_tokens(games):
    """games: movetext strings or token arrays -> (tokens uint64 [P], tok_off uint32 [n + 1])"""
    toks = [tokenize(g) if isinstance(g, (str, bytes)) else np.ascontiguousarray(g, np.uint64) for g in games]
    off = np.zeros(len(toks) + 1, np.uint32)
    off[1:] = np.cumsum([t.size for t in toks])
    flat = np.concatenate(toks) if toks and off[-1] else np.zeros(0, np.uint64)
    return flat, off


def encode_san_torch(games, winners=None, *, device, layout="reference", dist="legal", apply_mirror=False, engine=None, fens=None):
    """SAN games -> training tensors on the GPU in one call (sc_encode_san_device): every ply a row, dist one-hot on the move
    played (1 / (1 + 1e-5) there, as chess_encode_steps makes of a count of 1).
    games: movetext strings (tokenize) or token arrays, or the pair pack_tokens returns; winners: per game "white" / "black" /
    "draw" / None (read_games_csv's and read_pgn's second column).
    -> the dict encode_steps_torch returns (boards, meta, dist, dist_legal, legal_idx, n_legal, ply_off, status; layout and dist
    as there; outcome float32 [P] is White's result of the ply's game from winners, 0 without, negated under apply_mirror as
    everywhere) plus moves (torch int16 [P]: the move encoding, which stays below 2^15).  status: 0; -(i+1): token i names no legal move;
    100000 + i: it is ambiguous; 200000 + i: it is malformed.  score_torch, compare_torch, gather_batch_torch and
    ReplayBuffer.add take the dict as it is.
    fens: per game the position it starts from (read_pgn(setup=True)'s third list: FEN strings, None for the start position), or
    a scamd.fen.Positions of as many entries (sc_encode_san_device_from)."""
    from .fen import bases_of
    torch = _torch()
    L = lib()
    if isinstance(games, tuple) and len(games) == 2 and all(isinstance(a, np.ndarray) for a in games):
        flat, off = np.ascontiguousarray(games[0], np.uint64), np.ascontiguousarray(games[1], np.uint32)
    else:
        flat, off = pack_tokens(games)
    n = off.size - 1
    P = int(off[n])
    if winners is not None and len(winners) != n:
        raise ValueError(f"{len(winners)} winners for {n} games")
    dev = engine.device if engine is not None else device
    out, args = _device_outputs(torch, dev, P, n, layout, dist)
    moves = torch.empty(max(P, 1), dtype=torch.int16, device=torch.device("cuda", dev))
    pos, bidx, owned = bases_of(fens, n, dev)
    tok = flat if flat.size else np.zeros(1, np.uint64)
    if pos is None:
        _check(L.sc_encode_san_device(engine.h if engine else None, dev, n, _p(tok), _p(off), int(bool(apply_mirror)), args[0],
                                      _stream(torch, dev), *args[1:-1], _tp(moves), args[-1]))
    else:
        try:
            _check(L.sc_encode_san_device_from(engine.h if engine else None, dev, n, pos.h, _p(bidx), _p(tok), _p(off), int(bool(apply_mirror)),
                                               args[0], _stream(torch, dev), *args[1:-1], _tp(moves), args[-1]))
            if owned:
                torch.cuda.current_stream(dev).synchronize()   # the kernels read the set's records
        finally:
            if owned:
                pos.close()
    oc = np.zeros(n, np.float32) if winners is None else np.asarray([_WINNER[w.lower() if isinstance(w, str) else w] for w in winners], np.float32)
    res = _finish_outputs(torch, out, off, oc, apply_mirror, dev)
    res["moves"] = moves[:P]
    return res


def read_games_csv(path, limit=None):
    """The `moves` and `winner` columns of a game table like the reference's py/validation/sample.csv (its own use: limit=10)
    -> (list of movetext strings, list of winners)"""
    games, winners = [], []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if limit is not None and len(games) >= limit:
                break
            games.append(row["moves"])
            winners.append(row["winner"])
    return games, winners


_TAG = re.compile(r'^\s*\[\s*(\w+)\s+"((?:[^"\\]|\\.)*)"\s*\]\s*$')


def read_pgn(path, setup=False):
    """A PGN file -> (list of movetext strings, list of winners from [Result]): parse_pgn of its text; with setup=True a third
    list, the games' [FEN] headers"""
    with open(path, encoding="utf-8", errors="replace") as f:
        return parse_pgn(f.read(), setup=setup)


def parse_pgn(src, setup=False):
    """PGN text -> (list of movetext strings, list of winners from [Result]).  A game is a block of header tags and the movetext
    behind it; movetext without headers is a game too.  By default only games from the start position are read: a game with a
    [FEN] or a [SetUp "1"] header raises ValueError, which names the game.  setup=True reads those too and returns a third list:
    per game the text of its [FEN] header, None for a game from the start position (encode_san_torch's fens=)."""
    games, winners, fens = [], [], []
    tags, body = {}, []

    def close():
        mt = "\n".join(body).strip()
        if mt or tags:
            k = len(games) + 1
            name = f"game {k} ({tags.get('White', '?')} - {tags.get('Black', '?')})"
            if ("FEN" in tags or tags.get("SetUp") == "1") and not setup:
                raise ValueError(f"{name}: starts from a set-up position ([FEN] / [SetUp \"1\"]); only games from the start position can be read")
            if tags.get("SetUp") == "1" and "FEN" not in tags:
                raise ValueError(f"{name}: [SetUp \"1\"] without a [FEN] header")
            games.append(mt)
            winners.append(_RESULT.get(tags.get("Result")))
            fens.append(tags.get("FEN"))

    for ln in src.splitlines():
        m = _TAG.match(ln)
        if m and not (body and _open_comment("\n".join(body))):
            if body:   # a header block after movetext: the next game
                close()
                tags, body = {}, []
            tags[m.group(1)] = m.group(2)
        elif ln.strip() or body:
            body.append(ln)
    close()
    return (games, winners, fens) if setup else (games, winners)


def _open_comment(movetext):
    """is a {...} comment still open at the end of this movetext? (a tag-like line inside a comment is comment text)"""
    return movetext.rfind("{") > movetext.rfind("}")


def moves_to_san(games, fens=None, device=0):
    """Move lists (UCI strings or move ints) -> (list of lists of SAN strings, status int32 [n]) on the GPU, on torch's current
    stream (sc_moves_to_san_device): python-chess's Board.san() of every ply, check and mate marks included.  status[g]: 0, or
    -(i+1): move i of game g is not legal; that game's list ends in front of it.  fens: per game the position it starts from (FEN
    strings, None for the start position) or a scamd.fen.Positions."""
    from .fen import bases_of
    torch = _torch()
    L = lib()
    games = [list(g) for g in games]
    n = len(games)
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum([len(g) for g in games])
    P = int(off[n])
    flat = _moves([m for g in games for m in g])
    tdev = torch.device("cuda", device)
    tok = torch.zeros(max(P, 1), dtype=torch.int64, device=tdev)
    status = torch.zeros(max(n, 1), dtype=torch.int32, device=tdev)
    pos, bidx, owned = bases_of(fens, n, device)
    try:
        if pos is None:
            _check(L.sc_moves_to_san_device(device, n, _p(flat), _p(off), _stream(torch, device), _tp(tok), _tp(status)))
        else:
            _check(L.sc_moves_to_san_device_from(device, n, pos.h, _p(bidx), _p(flat), _p(off), _stream(torch, device), _tp(tok), _tp(status)))
        words = tok.cpu().numpy().view(np.uint64)   # (waits for the stream: the set's records have been read)
        st = status.cpu().numpy()[:n].copy()
    finally:
        if owned:
            pos.close()
    sans = []
    for g in range(n):
        row = []
        for t in words[off[g]:off[g + 1]]:
            if not t:
                break
            row.append(token_text(t))
        sans.append(row)
    return sans, st


def _as_tokens(tokens_or_sans):
    if isinstance(tokens_or_sans, np.ndarray):
        return np.ascontiguousarray(tokens_or_sans, np.uint64)
    out = np.zeros(len(tokens_or_sans), np.uint64)
    for i, w in enumerate(tokens_or_sans):
        raw = w.encode("latin-1") if isinstance(w, str) else int(w).to_bytes(8, "little")
        if len(raw) > 8:
            raise ValueError(f"{w!r} does not fit a token")
        out[i] = int.from_bytes(raw, "little")
    return out


def movetext(tokens_or_sans, fullmove=1, black_first=False, result=None):
    """SAN strings or tokens -> one line of movetext (sc_san_format; no GPU needed): "1. e4 e5 2. Nf3", with black_first
    "12... Nf6 13. d4"; result is appended as the last word; a token of 0 ends the moves."""
    L = lib()
    tok = _as_tokens(tokens_or_sans)
    res = None if result is None else result.encode()
    need = _count(L.sc_san_format(_p(tok) if tok.size else None, tok.size, int(fullmove), int(bool(black_first)), res, None, 0))
    buf = C.create_string_buffer(need + 1)
    _count(L.sc_san_format(_p(tok) if tok.size else None, tok.size, int(fullmove), int(bool(black_first)), res, buf, need + 1))
    return buf.value.decode("latin-1")


def wrap_movetext(text, width=80):
    """one line of movetext -> lines of at most `width` columns, broken at blanks"""
    lines, cur = [], ""
    for w in text.split(" "):
        if cur and len(cur) + 1 + len(w) > width:
            lines.append(cur)
            cur = w
        else:
            cur = cur + " " + w if cur else w
    return "\n".join(lines + [cur])


def _tag(name, value):
    return '[%s "%s"]\n' % (name, str(value).replace("\\", "\\\\").replace('"', '\\"'))


def write_pgn(path, games, results=None, headers=None, fens=None, append=False):
    """Games as lists of SAN strings (moves_to_san's) or token arrays -> a PGN file (no GPU needed).  results: per game "1-0" /
    "0-1" / "1/2-1/2" / None (written as *); headers: one dict for every game or a list of dicts (Event, Round, White, Black ...;
    Round defaults to the game's number); fens: per game the FEN it starts from or None: [SetUp "1"] and [FEN] are written and the
    move numbers follow the FEN.  Movetext lines of at most 80 columns, a blank line behind every game."""
    from .fen import parse_fen
    out = []
    for k, g in enumerate(games):
        h = dict((headers[k] if isinstance(headers, (list, tuple)) else headers) or {})
        res = (results[k] if results is not None else None) or "*"
        fen = fens[k] if fens is not None else None
        tags = {"Event": h.pop("Event", "?"), "Round": h.pop("Round", k + 1), "White": h.pop("White", "?"), "Black": h.pop("Black", "?"),
                "Result": res}
        tags.update(h)
        fullmove, black_first = 1, False
        if fen is not None:
            f = parse_fen(fen)
            fullmove, black_first = f.fullmove, f.turn == 0
            tags["SetUp"], tags["FEN"] = "1", fen
        out.append("".join(_tag(a, b) for a, b in tags.items()) + "\n" + wrap_movetext(movetext(g, fullmove, black_first, res)) + "\n\n")
    with open(path, "a" if append else "w", encoding="latin-1", newline="\n") as f:
        f.write("".join(out))
