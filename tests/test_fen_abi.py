"""Positions given as FEN, the checks that need no GPU: the entry points are declared, bound and exported and refuse without a
device; the host reader (sc_fen_parse) accepts and rejects what include/sc_engine.h says, field by field, and leaves the fields
the engine's own rules source makes of the same text; the readers of opening files and PGN studies hand the positions on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from lines import PERFT
from support import ROOT, scamd_built  # noqa: F401

PKG = os.path.join(ROOT, "smart-chess-rust_amd")
START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR"
REF39 = "1k1r4/1r5p/p4n1P/1ppP1P2/PP6/4PP1b/3B4/R1N1K3 b - - 0 39"
EPD = "r1bqkbnr/pppp1ppp/2n5/4p2Q/2B1P3/8/PPPP1PPP/RNB1K1NR w KQkq - bm Qxf7+; id \"scholar\";"
ACCEPTED = list(PERFT) + [REF39, EPD]
BOARD, TURN, CASTLING, EP, HALFMOVE, FULLMOVE = -1, -2, -3, -4, -5, -6

NEW_SYMBOLS = {"sc_fen_parse": 3, "sc_positions_from_fen": 5, "sc_positions_destroy": 1, "sc_positions_count": 1, "sc_positions_status": 2,
               "sc_positions_fen": 4, "sc_encode_positions_from": 13, "sc_encode_steps_device_from": 20, "sc_encode_san_device_from": 18,
               "sc_selfplay_set_position_from": 6, "sc_search_from": 15, "sc_selfplay_get_fen": 4, "sc_selfplay_set_openings_from": 7,
               "sc_selfplay_get_opening_fen": 4}


@pytest.fixture(scope="module")
def fen(scamd):
    import scamd.fen as m
    return m


@pytest.fixture(scope="module")
def H():
    """the host build of the engine's rules source, as tests/test_engine_rules_host.py builds it"""
    so = os.path.join(PKG, "lib", "libsc_rules_host.so")
    src = os.path.join(PKG, "csrc", "rules_host_api.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(os.path.join(PKG, "csrc", f))
                                                           for f in ("rules_host_api.cpp", "chess_rules.hpp", "chess_history.hpp")):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src])
    L = C.CDLL(so)
    L.sct_new.restype = C.c_void_p
    L.sct_free.restype = None
    L.sct_free.argtypes = [C.c_void_p]
    L.sct_set_fen.argtypes = [C.c_void_p, C.c_char_p]
    L.sct_get_fields.restype = None
    L.sct_get_fields.argtypes = [C.c_void_p, C.c_void_p]
    return L


def _parse(scamd, fen, text):
    """(return code, fields) of sc_fen_parse on exactly the bytes of `text`: the buffer holds no final zero"""
    raw = text if isinstance(text, bytes) else text.encode()
    buf = (C.c_char * max(len(raw), 1)).from_buffer_copy(raw or b"#")
    f = fen.FenFields()
    rc = scamd.lib().sc_fen_parse(C.cast(buf, C.c_char_p), len(raw), C.byref(f))
    return rc, f


def test_symbols_are_declared_bound_and_exported(scamd):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sc_engine.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", scamd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TW"}
    for name, arity in NEW_SYMBOLS.items():
        m = re.search(rf"\b{name}\s*\((.*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == arity == len(scamd.binding.ABI[name][1]), name
        assert name in exported, name


def test_names_live_in_the_submodule_only(scamd, fen):
    for name in ("Positions", "analyse", "parse_fen"):
        assert callable(getattr(fen, name)) and not hasattr(scamd, name), name
    assert C.sizeof(fen.FenFields) == 88


def test_entry_points_refuse_without_a_device(scamd, fen):
    L = scamd.lib()
    if L.sc_device_count() > 0:
        pytest.skip("a GPU is present")
    arr = (C.c_char_p * 1)(REF39.encode())
    h = C.c_void_p(1)
    status = np.zeros(1, np.int32)
    assert L.sc_positions_from_fen(0, 1, arr, C.byref(h), status.ctypes.data_as(C.c_void_p)) == -3 and not h.value
    assert "no HIP device" in L.sc_last_error().decode()
    off = np.zeros(2, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.sc_encode_positions_from(None, 0, 1, None, None, None, p(off), None, None, None, None, None, None) == -3
    assert L.sc_encode_steps_device_from(None, 0, 1, None, None, None, p(off), None, None, p(off), 0, 0, None, None, None, None, None, None,
                                         None, p(status)) == -3
    assert L.sc_encode_san_device_from(None, 0, 1, None, None, None, p(off), 0, 0, None, None, None, None, None, None, None, None, p(status)) == -3
    # the accessors of a set that does not exist, and the calls on handles that do not exist: errors, not crashes
    assert L.sc_positions_count(None) < 0 and L.sc_positions_status(None, 0) < -1 and L.sc_positions_fen(None, 0, None, 0) < 0
    L.sc_positions_destroy(None)
    buf = C.create_string_buffer(8)
    assert L.sc_selfplay_set_position_from(None, 0, None, 0, None, 0) < 0 and L.sc_selfplay_get_fen(None, 0, buf, 8) < 0
    assert L.sc_selfplay_set_openings_from(None, 1, None, None, None, p(off), None) < 0 and L.sc_selfplay_get_opening_fen(None, 0, buf, 8) < 0
    assert L.sc_search_from(None, None, 0, None, 0, 10, 2.5, 0, 0, 0, None, None, None, None, None) < 0
    with pytest.raises(scamd.EngineError, match="no HIP device"):
        fen.Positions([REF39])
    with pytest.raises(scamd.EngineError, match="no HIP device"):
        scamd.encode_positions([[]], fens=[REF39])
    with pytest.raises(scamd.EngineError, match="no HIP device"):
        fen.analyse(None, [REF39], 10, evaluator="synth")


@pytest.mark.parametrize("text", ACCEPTED + [None])
def test_accepted_fields_are_the_rules_sources(scamd, fen, H, text):
    """what sc_fen_parse leaves is what sct_set_fen (the engine's rules source, host build) makes of the same text; the castling
    field is compared as written, which for these positions is also the cleaned form"""
    text = text or START + " w KQkq - 0 1"
    rc, f = _parse(scamd, fen, text)
    assert rc == 0, text
    six = text if text != EPD else " ".join(EPD.split()[:4]) + " 0 1"   # an EPD record: halfmove 0, fullmove 1
    s = H.sct_new()
    assert H.sct_set_fen(s, six.encode()) == 0
    want = np.zeros(13, np.uint64)
    H.sct_get_fields(s, want.ctypes.data_as(C.c_void_p))
    H.sct_free(s)
    got = list(f.pcs) + list(f.occ) + [f.turn, f.castling, f.ep & 0xFFFFFFFFFFFFFFFF, f.halfmove, f.fullmove]
    assert [int(x) for x in got] == [int(x) for x in want], text
    assert f.reserved == 0


def test_accepted_forms(scamd, fen):
    rc, f = _parse(scamd, fen, START + " b Kq a3 12 0")
    assert (rc, f.turn, f.castling, f.ep, f.halfmove, f.fullmove) == (0, 0, 1 | 8, 16, 12, 1)    # fullmove 0 is read as 1
    rc, f = _parse(scamd, fen, "  " + START + "\tw\t-\th6\t65535\t65535\n")
    assert (rc, f.castling, f.ep, f.halfmove, f.fullmove) == (0, 0, 47, 65535, 65535)
    # the four fields of an EPD record; what follows them is ignored unless it is two integers
    for tail in ("", " bm Qh5;", " 7", " 7 bm", " bm 7 8", " hmvc 3; fmvn 9;"):
        rc, f = _parse(scamd, fen, START + " w KQkq -" + tail)
        assert (rc, f.halfmove, f.fullmove) == (0, 0, 1), tail
    assert _parse(scamd, fen, START + " w QK -")[0] == 0 and _parse(scamd, fen, START + " w qk -")[1].castling == 12


REJECTED = [
    ("seven ranks", "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP w KQkq - 0 1", BOARD),
    ("nine ranks", START + "/8 w KQkq - 0 1", BOARD),
    ("a rank summing to 9", "rnbqkbnr/pppppppp/9/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1", BOARD),
    ("a rank of 8 + 1", "rnbqkbnr/pppppppp/8p/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1", BOARD),
    ("a rank summing to 7", "rnbqkbnr/pppppppp/7/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1", BOARD),
    ("44 in a rank", "rnbqkbnr/pppppppp/44/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1", BOARD),
    ("an x piece", "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNx w KQkq - 0 1", BOARD),
    ("turn W", START + " W KQkq - 0 1", TURN),
    ("turn ww", START + " ww KQkq - 0 1", TURN),
    ("castling KQkqK", START + " w KQkqK - 0 1", CASTLING),
    ("castling HAha", START + " w HAha - 0 1", CASTLING),
    ("castling kK", START + " w kK - 0 1", CASTLING),
    ("castling KK", START + " w KK - 0 1", CASTLING),
    ("ep e4", START + " w KQkq e4 0 1", EP),
    ("ep e", START + " w KQkq e 0 1", EP),
    ("ep i3", START + " w KQkq i3 0 1", EP),
    ("halfmove -1", START + " w KQkq - -1 1", HALFMOVE),
    ("halfmove 70000", START + " w KQkq - 70000 1", HALFMOVE),
    ("fullmove -1", START + " w KQkq - 0 -1", FULLMOVE),
    ("fullmove 70000", START + " w KQkq - 0 70000", FULLMOVE),
    ("a clock of 30 digits", START + " w KQkq - 0 " + "9" * 30, FULLMOVE),
    ("an empty string", "", BOARD),
    ("white space alone", " \t\n", BOARD),
]


@pytest.mark.parametrize("what,text,code", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejected_with_the_code_of_the_field(scamd, fen, what, text, code):
    rc, f = _parse(scamd, fen, text)
    assert rc == code, (what, rc)
    assert bytes(f) == bytes(C.sizeof(f)), "a refused text leaves zeroed fields"
    assert fen.FIELDS[-code - 1] in scamd.lib().sc_last_error().decode()
    with pytest.raises(ValueError, match=fen.FIELDS[-code - 1]):
        fen.parse_fen(text)


def test_a_text_cut_inside_each_field(scamd, fen):
    """`len` bounds the read: a cut inside the board, the turn, the castling or the ep field fails as the field that is then
    malformed or missing; behind the ep field the record is an EPD one, and a cut can only shorten or drop the clocks"""
    text = "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq e6 12 34"
    board, end = text.index(" "), len(text)
    want = {}
    for n in range(end + 1):
        if n < board:
            want[n] = BOARD                              # inside the board
        elif n <= board + 1:
            want[n] = TURN                               # the board alone
        elif n <= text.index("KQkq"):
            want[n] = CASTLING                           # "... w" / "... w "
        elif n <= text.index("e6"):
            want[n] = EP                                 # "... w K" is a castling field: the ep field is missing
        elif n == text.index("e6") + 1:
            want[n] = EP                                 # "e"
        else:
            want[n] = 0
    got = {n: _parse(scamd, fen, text[:n])[0] for n in range(end + 1)}
    assert got == want
    # ... the shortened clocks: "1" for "12" needs its partner, "12 3" is two integers
    assert [(_parse(scamd, fen, text[:n])[1].halfmove, _parse(scamd, fen, text[:n])[1].fullmove) for n in (end - 5, end - 3, end - 2, end - 1, end)] == \
        [(0, 1), (0, 1), (0, 1), (12, 3), (12, 34)]
    # a zero byte is no white space and no piece
    assert _parse(scamd, fen, b"8/8/8/8/8/8/4K3/4k3\0w - - 0 1")[0] == BOARD


def test_read_openings_mixes_fen_lines_and_plain_lines(scamd, tmp_path):
    from scamd.selfplay import read_openings
    p = tmp_path / "openings.txt"
    p.write_text("# a suite\n"
                 "e2e4 e7e5 g1f3\n"
                 f"fen {REF39} moves h3g2 a1a2   # the reference's position\n"
                 "\n"
                 "fen 8/2p5/3p4/KP5r/1R3p1k/8/4P1P1/8 w - -\n"
                 f"fen {START} w KQkq - 0 1 moves\n"
                 "d2d4\n")
    assert read_openings(str(p)) == [["e2e4", "e7e5", "g1f3"], (REF39, ["h3g2", "a1a2"]), [], ("8/2p5/3p4/KP5r/1R3p1k/8/4P1P1/8 w - -", []),
                                     (START + " w KQkq - 0 1", []), ["d2d4"]]
    p.write_text(f"fen {START} w KQkq e4 0 1 moves e2e4\n")
    with pytest.raises(ValueError, match=r"openings.txt:1: bad FEN \(ep field\)"):
        read_openings(str(p))
    p.write_text(f"e2e4\nfen {START} w KQkq\n")
    with pytest.raises(ValueError, match=r"openings.txt:2: a FEN of 4 or 6 fields"):
        read_openings(str(p))
    p.write_text(f"fen {REF39} moves h3g2 Ra2\n")
    with pytest.raises(ValueError, match="'Ra2' is not a UCI move"):
        read_openings(str(p))


def test_cli_reader_checks_fen_lines_before_it_needs_a_gpu(scamd, tmp_path):
    """lib/sc-play reads the same file format; a malformed FEN is reported with its line before any device is looked for"""
    exe = os.path.join(PKG, "lib", "sc-play")
    p = tmp_path / "openings.txt"
    p.write_text(f"e2e4\nfen {START} w KQkqK - 0 1 moves e2e4\n")
    r = subprocess.run([exe, "--white-device", "cuda", "--black-type", "nn", "--openings", str(p)], capture_output=True, text=True)
    assert r.returncode == 2 and "openings.txt:2:" in r.stderr and "castling" in r.stderr, r.stderr


def test_read_pgn_setup(scamd, tmp_path):
    import scamd.san as san
    one = '[Event "Casual"]\n[White "Anderssen"]\n[Black "Kieseritzky"]\n[Result "1-0"]\n\n1. e4 e5 2. f4 exf4 1-0\n'
    two = '[Event "Study"]\n[White "Composer"]\n[Black "Nobody"]\n[Result "*"]\n[SetUp "1"]\n[FEN "8/8/8/8/8/8/4K3/4k3 w - - 0 1"]\n\n1. Kd3 *\n'
    p = tmp_path / "games.pgn"
    p.write_text(one + "\n" + two)
    with pytest.raises(ValueError, match=r"game 2 \(Composer - Nobody\)"):
        san.read_pgn(str(p))                                   # the default refuses set-up games, as before
    games, winners, fens = san.read_pgn(str(p), setup=True)
    assert fens == [None, "8/8/8/8/8/8/4K3/4k3 w - - 0 1"] and winners == ["white", None] and len(games) == 2
    assert [int(t) for t in san.tokenize(games[1])] == [int.from_bytes(b"Kd3".ljust(8, b"\0"), "little")]
    assert san.parse_pgn("1. e4 e5 *", setup=True) == (["1. e4 e5 *"], [None], [None])
    with pytest.raises(ValueError, match="without a \\[FEN\\]"):
        san.parse_pgn('[SetUp "1"]\n\n1. e4 *', setup=True)
