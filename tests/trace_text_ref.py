"""The reference reader of trace files, in pure Python: json.loads decides whether the text is JSON at all, a small tokenizer of
its own gives every value its byte offset, and the shape, move, count and limit rules of include/sc_engine.h (sc_traces_read) give
the arrays or (code, err_at).  Every defect is collected as (offset, code); the smallest pair wins, as on the device.
Text holding `true` / `false`, or a backslash outside a string, is outside what this reader judges: ValueError, as for text that
json.loads refuses for a reason the contract does not list."""
import json
import re

import numpy as np

UNBALANCED, ESCAPE, STEPS, SHAPE, MOVE, COUNT, CHILDREN, PLIES, OUTCOME, SPACE = range(1, 11)
MAX_PLIES, MAX_CHILDREN, MAX_COUNT, MAX_FEN = 4000, 224, 4294967295, 127
TERMINATION_NAMES = ("", "Checkmate", "Stalemate", "InsufficientMaterial", "SeventyfiveMoves", "FivefoldRepetition", "FiftyMoves",
                     "ThreefoldRepetition", "VariantWin", "VariantLoss", "VariantDraw")
_WS = b" \t\n\r"
_UCI = re.compile(rb"[a-h][1-8][a-h][1-8][nbrq]?\Z")
_PROMO = {b"n": 2, b"b": 3, b"r": 4, b"q": 5}


def uci_move(s):
    f = (s[1] - 49) * 8 + s[0] - 97
    t = (s[3] - 49) * 8 + s[2] - 97
    return f | (t << 6) | ((_PROMO[s[4:5]] if len(s) > 4 else 0) << 12)


class Node:
    """kind: "obj" (value: [(key bytes, offset of the key's quote, Node)]), "arr" ([Node]), "str" (bytes), "tok" (the raw bytes of
    a number or null); at: the offset of its first byte"""
    __slots__ = ("kind", "value", "at")

    def __init__(self, kind, value, at):
        self.kind, self.value, self.at = kind, value, at


def _skip(b, i):
    while i < len(b) and b[i] in _WS:
        i += 1
    return i


def _string(b, i):
    j = b.index(b'"', i + 1)
    return b[i + 1:j], j + 1


def _value(b, i):
    """the value at b[i] (text json.loads has accepted, without escapes) -> (Node, offset behind it); iterative over containers"""
    root = Node("arr", [], -1)
    stack = [root]
    key = None
    while True:
        i = _skip(b, i)
        c = b[i:i + 1]
        top = stack[-1]
        if c in (b"]", b"}"):
            stack.pop()
            i += 1
        elif c == b",":
            i += 1
            continue
        elif c == b":":
            i += 1
            continue
        else:
            if top.kind == "obj" and key is None:
                s, j = _string(b, i)
                key = (s, i)
                i = j
                continue
            if c == b"[":
                node = Node("arr", [], i)
                i += 1
            elif c == b"{":
                node = Node("obj", [], i)
                i += 1
            elif c == b'"':
                s, j = _string(b, i)
                node = Node("str", s, i)
                i = j
            else:
                j = i
                while j < len(b) and b[j] not in b" \t\n\r,]}":
                    j += 1
                node = Node("tok", b[i:j], i)
                i = j
            if top.kind == "obj":
                top.value.append((key[0], key[1], node))
                key = None
            else:
                top.value.append(node)
            if node.kind in ("arr", "obj"):
                stack.append(node)
        if len(stack) == 1:
            return root.value[0], i


def _lexical(b):
    """the defects a byte scan finds: (offset, code) of every one"""
    out, depth, in_str, first = [], 0, False, True
    for i, c in enumerate(b):
        if in_str:
            if c == 0x22:
                in_str = False
            elif c == 0x5C:
                out.append((i, ESCAPE))
            continue
        if c in _WS:
            continue
        if first and c != 0x7B:
            out.append((i, UNBALANCED))
        first = False
        if c == 0x22:
            in_str = True
        elif c in b"[{":
            depth += 1
        elif c in b"]}":
            depth -= 1
            if depth < 0:
                out.append((i, UNBALANCED))
        elif c == 0x5C:
            raise ValueError("a backslash outside a string")
    if in_str or depth != 0 or first:
        out.append((len(b), UNBALANCED))
    return out


def _move(node, bad):
    if not _UCI.match(node.value):
        bad.append((node.at, MOVE))
        return 0
    return uci_move(node.value)


def read_one(data):
    """one file's bytes -> dict(status, err_at, moves [uint16], children [[(move, count)] per ply], opening [uint16],
    outcome (has_outcome, termination, winner), fen str or None).  status 0, or -code with err_at; a refused file has no arrays"""
    b = bytes(data)
    bad = _lexical(b)
    res = dict(status=0, err_at=0, moves=[], children=[], opening=[], outcome=(0, 0, -1), fen=None)

    def refused():
        at, code = min(bad)
        return dict(res, status=-code, err_at=at, moves=[], children=[], opening=[], outcome=(0, 0, -1), fen=None)

    if bad:
        return refused()
    text = b.decode("latin-1")
    if re.search(r"\b(true|false)\b", re.sub(r'"[^"]*"', '""', text)):
        raise ValueError("true / false: outside the contract")
    try:
        json.loads(text)
    except ValueError as e:
        raise ValueError(f"not JSON, for a reason the contract does not list: {e}") from e
    top, _ = _value(b, 0)
    members = {}
    for key, at, node in top.value:
        members.setdefault(key, []).append((at, node))
    for key in (b"outcome", b"opening", b"fen"):
        if len(members.get(key, [])) > 1:
            raise ValueError(f"two {key!r} members: outside the contract")
    steps = members.get(b"steps", [])
    if not steps:
        bad.append((len(b), STEPS))
    for at, _ in steps[1:]:
        bad.append((at, STEPS))
    if steps and steps[0][1].kind != "arr":
        bad.append((steps[0][0], STEPS))
    elif steps:
        for i, st in enumerate(steps[0][1].value):
            if i >= MAX_PLIES:
                bad.append((st.at, PLIES))
            if st.kind != "arr" or not st.value or st.value[0].kind != "str":
                bad.append((st.at, SHAPE))
                continue
            res["moves"].append(_move(st.value[0], bad))
            if len(st.value) != 3 or st.value[1].kind != "tok" or st.value[2].kind != "arr":
                bad.append((st.at, SHAPE))
                res["children"].append([])
                continue
            row = []
            for k, ch in enumerate(st.value[2].value):
                if k >= MAX_CHILDREN:
                    bad.append((ch.at, CHILDREN))
                if ch.kind != "arr" or not ch.value or ch.value[0].kind != "str" or len(ch.value) < 2:
                    bad.append((ch.at, SHAPE))
                    continue
                mv, cnt = _move(ch.value[0], bad), ch.value[1]
                if cnt.kind != "tok" or not re.fullmatch(rb"[0-9]+", cnt.value) or int(cnt.value) > MAX_COUNT:
                    bad.append((cnt.at, COUNT))
                    continue
                row.append((mv, int(cnt.value)))
            res["children"].append(row)
    if b"outcome" in members:
        at, oc = members[b"outcome"][0]
        ok = oc.kind == "tok" and oc.value == b"null"
        if oc.kind == "obj" and sorted(k for k, _, _ in oc.value) == [b"termination", b"winner"]:
            m = {k: v for k, _, v in oc.value}
            t, w = m[b"termination"], m[b"winner"]
            name = t.value.decode("latin-1") if t.kind == "str" else None
            wv = {b"White": 1, b"Black": 0}.get(w.value) if w.kind == "str" else (-1 if w.value == b"null" and w.kind == "tok" else None)
            if name in TERMINATION_NAMES[1:] and wv is not None:
                ok, res["outcome"] = True, (1, TERMINATION_NAMES.index(name), wv)
        if not ok:
            bad.append((at, OUTCOME))
    if b"opening" in members:
        at, op = members[b"opening"][0]
        if op.kind != "arr":
            raise ValueError('"opening" is not an array: outside the contract')
        for el in op.value:
            if el.kind != "str":
                bad.append((el.at, SHAPE))
            else:
                res["opening"].append(_move(el, bad))
    if b"fen" in members:
        at, fen = members[b"fen"][0]
        if fen.kind != "str":
            raise ValueError('"fen" is not a string: outside the contract')
        if len(fen.value) > MAX_FEN:
            bad.append((fen.at, SHAPE))
        res["fen"] = fen.value.decode("latin-1")
    return refused() if bad else res


def read_many(blobs):
    """the files of one call -> the packed arrays and summary fields sc_traces_summary / sc_traces_get give, as numpy"""
    one = [read_one(b) for b in blobs]
    n = len(one)
    out = dict(status=np.array([r["status"] for r in one], np.int32).reshape(n), err_at=np.array([r["err_at"] for r in one], np.uint32).reshape(n),
               n_steps=np.array([len(r["moves"]) for r in one], np.uint32).reshape(n),
               n_children=np.array([sum(len(c) for c in r["children"]) for r in one], np.uint32).reshape(n),
               n_opening=np.array([len(r["opening"]) for r in one], np.uint32).reshape(n),
               outcome=np.array([r["outcome"] for r in one], np.int32).reshape(n, 3),
               has_fen=np.array([int(r["fen"] is not None) for r in one], np.int32).reshape(n), fens=[r["fen"] for r in one])
    out["move_off"] = np.concatenate([[0], np.cumsum(out["n_steps"], dtype=np.uint64)]).astype(np.uint32)
    out["open_off"] = np.concatenate([[0], np.cumsum(out["n_opening"], dtype=np.uint64)]).astype(np.uint32)
    out["moves"] = np.array([m for r in one for m in r["moves"]], np.uint16)
    rows = [c for r in one for c in r["children"]]
    out["child_off"] = np.concatenate([[0], np.cumsum([len(c) for c in rows], dtype=np.uint64)]).astype(np.uint32)
    out["child_mv"] = np.array([m for c in rows for m, _ in c], np.uint16)
    out["child_n"] = np.array([k for c in rows for _, k in c], np.uint32)
    out["opening"] = np.array([m for r in one for m in r["opening"]], np.uint16)
    return out
