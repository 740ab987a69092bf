"""SAN game records, the checks that need no GPU: the two entry points are declared, bound and exported, the device one refuses
without a device, and the host tokenizer (sc_san_tokenize) and the readers of scamd.san do what include/sc_engine.h says."""
import csv
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from support import GOLD, ROOT, scamd_built  # noqa: F401

RESERVED = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def san(scamd):
    import scamd.san as m
    return m


def _tok(s):
    return int.from_bytes(s.encode().ljust(8, b"\0"), "little")


def _toks(san, text):
    return [int(t) for t in san.tokenize(text)]


def test_symbols_are_declared_bound_and_exported(scamd):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sc_engine.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", scamd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TW"}
    for name, arity in (("sc_san_tokenize", 5), ("sc_encode_san_device", 16)):
        m = re.search(rf"\b{name}\s*\((.*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == arity == len(scamd.binding.ABI[name][1]), name
        assert name in exported, name


def test_names_live_in_the_submodule_only(scamd, san):
    for name in ("tokenize", "encode_san_torch", "read_games_csv", "read_pgn"):
        assert callable(getattr(san, name)) and not hasattr(scamd, name), name


def test_device_entry_point_refuses_without_a_device(scamd):
    L = scamd.lib()
    if L.sc_device_count() > 0:
        pytest.skip("a GPU is present")
    tokens, off, status = np.array([_tok("e4")], np.uint64), np.array([0, 1], np.uint32), np.zeros(1, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = L.sc_encode_san_device(None, 0, 1, p(tokens), p(off), 0, 0, None, None, None, None, None, None, None, None, p(status))
    assert rc == -3 and "no HIP device" in L.sc_last_error().decode()
    import scamd.san
    with pytest.raises(scamd.EngineError, match="no HIP device"):
        scamd.san.encode_san_torch(["1. e4"], device=0)


def test_tokenizer_move_numbers(san):
    want = [_tok(s) for s in ("e4", "e5", "Nf3", "Nc6")]
    assert _toks(san, "1. e4 e5 2. Nf3 Nc6") == want
    assert _toks(san, "1.e4 e5 2.Nf3 Nc6") == want                  # glued
    assert _toks(san, "1. e4 1... e5 2. Nf3 2...Nc6") == want       # black's number, apart and glued
    assert _toks(san, "1. e4 1. ... e5 2 Nf3 Nc6") == want          # dots on their own, a number without a dot


def test_tokenizer_comments_variations_nags(san):
    text = "1. e4 {best by test} e5 (1... c5 (1... e6 {the ) French} 2. d4) 2. Nf3) 2. Nf3 $1 Nc6 $14 ; Bb5 is next\n3. Bb5 a6"
    assert _toks(san, text) == [_tok(s) for s in ("e4", "e5", "Nf3", "Nc6", "Bb5", "a6")]
    assert _toks(san, "e4 ; e5 d4\nd5") == [_tok("e4"), _tok("d5")]
    assert _toks(san, "e4 {never closed e5 d4") == [_tok("e4")]
    assert _toks(san, "e4 (never closed e5 d4") == [_tok("e4")]
    assert _toks(san, '[Event "a ] in a value"]\n[Site "?"] 1. d4 d5') == [_tok("d4"), _tok("d5")]


@pytest.mark.parametrize("result", ["1-0", "0-1", "1/2-1/2", "*"])
def test_tokenizer_stops_at_the_result(san, result):
    assert _toks(san, f"1. e4 e5 {result} 2. Nf3") == [_tok("e4"), _tok("e5")]
    assert _toks(san, result) == []


def test_tokenizer_suffixes_and_castling(san):
    assert _toks(san, "Nf3!?+ Qxf7#!! e8=Q+ exd8=N# O-O+ O-O-O# 0-0 0-0-0 e4?? !") == \
        [_tok(s) for s in ("Nf3", "Qxf7", "e8=Q", "exd8=N", "O-O", "O-O-O", "0-0", "0-0-0", "e4")]
    assert _tok("Nbd2") == 0x3264624E   # first character in the lowest byte


def test_tokenizer_reserved_value_keeps_the_ply_count(san):
    got = _toks(san, "1. e4 Ng1xf3=Q 2. d4 ) d5 Qa1xh8+")
    assert got == [_tok("e4"), RESERVED, _tok("d4"), RESERVED, _tok("d5"), _tok("Qa1xh8")]
    assert _toks(san, "exd8=Q+!") == [_tok("exd8=Q")]      # 7 characters fit
    assert _toks(san, "Qa1xh8=Q") == [RESERVED]            # 8 do not


def test_tokenizer_empty_and_capacity(scamd, san):
    L = scamd.lib()
    assert _toks(san, "") == [] and _toks(san, "  \n {only a comment} ") == []
    n = C.c_uint32(77)
    assert L.sc_san_tokenize(None, 0, None, 0, C.byref(n)) == 0 and n.value == 0
    text = b"1. e4 e5 2. Nf3 Nc6 3. Bb5 a6"
    buf = np.full(8, 0x5a5a5a5a5a5a5a5a, np.uint64)
    rc = L.sc_san_tokenize(text, len(text), buf.ctypes.data_as(C.c_void_p), 4, C.byref(n))
    assert rc < 0 and rc == san.ERR_CAPACITY and n.value == 6
    assert buf[:4].tolist() == [_tok(s) for s in ("e4", "e5", "Nf3", "Nc6")] and (buf[4:] == 0x5a5a5a5a5a5a5a5a).all()
    assert L.sc_san_tokenize(text, len(text), None, 0, C.byref(n)) == san.ERR_CAPACITY and n.value == 6    # the count query
    assert L.sc_san_tokenize(text, 8, buf.ctypes.data_as(C.c_void_p), 8, C.byref(n)) == 0 and n.value == 2   # len bounds the read
    assert L.sc_san_tokenize(text, len(text), None, 4, C.byref(n)) == -1 and L.sc_san_tokenize(text, len(text), None, 0, None) == -1
    assert san.tokenize("e4 " * 500).size == 500      # the binding grows its buffer


def test_read_games_csv_golden(san):
    path = os.path.join(GOLD, "ref_sample_games.csv")
    games, winners = san.read_games_csv(path)
    rows = list(csv.DictReader(open(path, newline="")))
    assert len(games) == len(winners) == 60
    assert [san.tokenize(g).size for g in games] == [int(r["turns"]) for r in rows]
    assert set(winners) <= {"white", "black", "draw"} and winners == [r["winner"] for r in rows]
    assert all(int(t) != RESERVED for g in games for t in san.tokenize(g))
    g10, w10 = san.read_games_csv(path, limit=10)
    assert g10 == games[:10] and w10 == winners[:10]
    flat, off = san.pack_tokens(games)
    assert flat.dtype == np.uint64 and off.dtype == np.uint32 and off[-1] == flat.size == sum(int(r["turns"]) for r in rows)


def test_read_pgn(san, tmp_path):
    one = '[Event "Casual"]\n[White "Anderssen"]\n[Black "Kieseritzky"]\n[Result "1-0"]\n\n1. e4 e5 2. f4 exf4 {[%clk 0:01]\n[not a tag]}\n3. Bc4 Qh4+ 1-0\n'
    two = '[Event "Study"]\n[White "Composer"]\n[Black "Nobody"]\n[Result "*"]\n[SetUp "1"]\n[FEN "8/8/8/8/8/8/4K3/4k3 w - - 0 1"]\n\n1. Kd3 *\n'
    three = '[Event "Third"]\n[Result "1/2-1/2"]\n\n1. d4 d5 1/2-1/2\n'
    p = tmp_path / "games.pgn"
    p.write_text(one + "\n" + three)
    games, winners = san.read_pgn(str(p))
    assert winners == ["white", "draw"] and len(games) == 2
    assert [int(t) for t in san.tokenize(games[0])] == [_tok(s) for s in ("e4", "e5", "f4", "exf4", "Bc4", "Qh4")]
    assert [int(t) for t in san.tokenize(games[1])] == [_tok("d4"), _tok("d5")]
    p.write_text(one + "\n" + two)
    with pytest.raises(ValueError, match=r"game 2 \(Composer - Nobody\)"):
        san.read_pgn(str(p))
    p.write_text('[Event "x"]\n[FEN "8/8/8/8/8/8/4K3/4k3 w - - 0 1"]\n\n1. Kd3 *\n')
    with pytest.raises(ValueError, match="game 1"):
        san.read_pgn(str(p))
    assert san.parse_pgn("1. e4 e5 *") == (["1. e4 e5 *"], [None])
