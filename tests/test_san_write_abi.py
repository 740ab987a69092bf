"""Games written as SAN and PGN, the checks that need no GPU: the host formatter (sc_san_format), scamd.san.movetext / write_pgn
read back by the existing tokenizer and PGN reader, the device entry points' argument checks, and sc-play's --pgn flag."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from support import ROOT, scamd_built  # noqa: F401

PLAY = os.path.join(ROOT, "smart-chess-rust_amd", "lib", "sc-play")
NEW = (("sc_moves_to_san_device", 7), ("sc_moves_to_san_device_from", 9), ("sc_san_format", 7), ("sc_selfplay_write_pgn", 8))


@pytest.fixture(scope="module")
def san(scamd):
    import scamd.san as m
    return m


def _tok(s):
    return int.from_bytes(s.encode().ljust(8, b"\0"), "little")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _format(L, words, fullmove=1, black_first=0, result=None, cap=256):
    """sc_san_format into a buffer of `cap` bytes behind which 8 guard bytes stand -> (return value, the buffer's text)"""
    tok = np.asarray([w if isinstance(w, int) else _tok(w) for w in words] or [0], np.uint64)
    buf = C.create_string_buffer(b"\x5a" * (cap + 8), cap + 8)
    rc = L.sc_san_format(_p(tok), len(words), fullmove, black_first, result, buf, cap)
    assert buf.raw[cap:] == b"\x5a" * 8, "written past cap"
    return rc, (buf.raw[:cap].split(b"\0")[0].decode() if cap else "")


def _whole(text):
    """what a call with room for the whole text gives: its length and the text"""
    return len(text), text


def test_symbols_are_declared_bound_and_exported(scamd):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sc_engine.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", scamd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TW"}
    for name, arity in NEW:
        m = re.search(rf"\b{name}\s*\((.*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == arity == len(scamd.binding.ABI[name][1]), name
        assert name in exported, name


def test_names_live_in_the_submodule_only(scamd, san):
    for name in ("moves_to_san", "movetext", "write_pgn"):
        assert callable(getattr(san, name)) and not hasattr(scamd, name), name
    assert callable(scamd.SelfPlay.write_pgn)


def test_format_white_first_black_first_result(scamd):
    L = scamd.lib()
    assert _format(L, ["e4", "e5", "Nf3"]) == _whole("1. e4 e5 2. Nf3")
    assert _format(L, ["Nf6", "d4", "d5", "c4"], 12, 1) == _whole("12... Nf6 13. d4 d5 14. c4")
    assert _format(L, ["e4", "e5"], result=b"1/2-1/2") == _whole("1. e4 e5 1/2-1/2")
    assert _format(L, ["Qh4xe1+", "exd8=Q#", "O-O-O"], 9, 1, b"*") == _whole("9... Qh4xe1+ 10. exd8=Q# O-O-O *")   # the suffix is the token's
    assert _format(L, ["Nf6"], 12, 1) == _whole("12... Nf6")


def test_format_empty_list_and_zero_token(scamd):
    L = scamd.lib()
    assert _format(L, []) == _whole("")
    assert _format(L, [], result=b"1-0") == _whole("1-0")
    assert L.sc_san_format(None, 0, 1, 0, None, None, 0) == 0
    assert _format(L, ["e4", "e5", 0, "Nf3"]) == _whole("1. e4 e5")            # a token of 0 ends the text
    assert _format(L, [0, "e4"], result=b"0-1") == _whole("0-1")


def test_format_every_cap(scamd):
    """a cap too small: the needed length is returned, a terminated prefix is written and nothing behind it"""
    L = scamd.lib()
    words, whole = ["e4", "e5", "Nf3", "Nc6", "Bb5"], "1. e4 e5 2. Nf3 Nc6 3. Bb5 1-0"
    for cap in range(0, len(whole) + 3):
        rc, text = _format(L, words, result=b"1-0", cap=cap)
        assert rc == len(whole) and text == whole[:max(cap - 1, 0)], cap
    tok = np.asarray([_tok("e4")], np.uint64)
    assert L.sc_san_format(None, 1, 1, 0, None, None, 0) == -1 and L.sc_san_format(_p(tok), 1, 1, 0, None, None, 4) == -1
    assert L.sc_san_format(_p(tok), 1, -1, 0, None, None, 0) == -1


def test_movetext_reads_back_through_the_tokenizer(san):
    words = ["e4", "e5", "Nf3+", "Nbd7", "exd8=Q#", "O-O-O+", "R1e2", "Qh4xe1+"]
    for fullmove, black in ((1, False), (12, True), (99, False)):
        text = san.movetext(words, fullmove, black, "1-0")
        assert text.startswith("12... e4 13. e5" if black else "%d. e4 e5" % fullmove) and text.endswith(" 1-0")
        assert [san.token_text(t) for t in san.tokenize(text)] == [w.rstrip("+#") for w in words]
    tokens = np.asarray([_tok(w) for w in words], np.uint64)
    assert san.movetext(tokens) == san.movetext(words)          # tokens or strings
    assert san.movetext([]) == "" and san.movetext([], result="*") == "*"
    with pytest.raises(ValueError):
        san.movetext(["Qh4xe1+!!"])


def test_write_pgn_reads_back(san, tmp_path):
    fen = "r1bqkbnr/pppp1ppp/2n5/4p3/4P3/5N2/PPPP1PPP/RNBQKB1R b KQkq - 2 12"
    long_game = ["Nf3", "Nf6", "Ng1", "Ng8"] * 40
    games = [["e4", "e5", "Nf3", "Nc6", "Bb5+"], ["Nf6", "d4", "exd4"], long_game, []]
    path = str(tmp_path / "out.pgn")
    san.write_pgn(path, games[:2], results=["1-0", None], headers={"Event": 'a "quoted" \\ name', "White": "new", "Black": "old"},
                  fens=[None, fen])
    san.write_pgn(path, games[2:], results=["1/2-1/2", "0-1"], headers=[{"White": "x", "Termination": "FiftyMoves"}, {}], append=True)
    text = open(path).read()
    assert all(len(ln) <= 80 for ln in text.splitlines()) and max(len(ln) for ln in text.splitlines()) > 70
    assert text.count("[Event ") == 4 and text.count('[SetUp "1"]') == 1 and text.count("[FEN ") == 1 and text.endswith("\n\n")
    assert '[Event "a \\"quoted\\" \\\\ name"]' in text and '[Termination "FiftyMoves"]' in text
    assert re.search(r'\[FEN "%s"\]\n\n12\.\.\. Nf6 13\. d4 exd4 \*\n' % re.escape(fen), text)
    got, winners, fens = san.read_pgn(path, setup=True)
    assert winners == ["white", None, "draw", "black"] and fens == [None, fen, None, None]
    assert [[san.token_text(t) for t in san.tokenize(g)] for g in got] == [[w.rstrip("+#") for w in g] for g in games]
    san.write_pgn(path, [["d4"]])                       # without append the file starts again
    assert san.read_pgn(path) == (["1. d4 *"], [None]) and '[Round "1"]' in open(path).read()


def test_device_entry_points_check_their_arguments(scamd):
    L = scamd.lib()
    moves, off, host = np.array([796], np.uint16), np.array([0, 1], np.uint32), np.zeros(8, np.int64)
    # NULL status / tokens / offsets are refused before the device is looked at, as in sc_encode_steps_device
    assert L.sc_moves_to_san_device(0, 1, _p(moves), _p(off), None, _p(host), None) == -1
    assert L.sc_moves_to_san_device(0, 1, _p(moves), _p(off), None, None, _p(host)) == -1
    assert L.sc_moves_to_san_device(0, 1, _p(moves), None, None, _p(host), _p(host)) == -1
    assert L.sc_moves_to_san_device(0, -1, _p(moves), _p(off), None, _p(host), _p(host)) == -1
    assert L.sc_moves_to_san_device_from(0, 1, None, None, _p(moves), _p(off), None, None, _p(host)) == -1
    assert L.sc_selfplay_write_pgn(None, 0, None, b"x.pgn", 0, None, None, None) == -1


def test_device_entry_points_refuse_without_a_device(scamd):
    L = scamd.lib()
    moves, off, host = np.array([796], np.uint16), np.array([0, 1], np.uint32), np.zeros(8, np.int64)
    if L.sc_device_count() > 0:
        pytest.skip("a GPU is present")
    assert L.sc_moves_to_san_device(0, 1, _p(moves), _p(off), None, _p(host), _p(host)) == -3 and "no HIP device" in L.sc_last_error().decode()
    assert L.sc_moves_to_san_device_from(0, 1, None, None, _p(moves), _p(off), None, _p(host), _p(host)) == -3
    import scamd.san
    with pytest.raises(scamd.EngineError, match="no HIP device"):
        scamd.san.moves_to_san([["e2e4"]])


def test_play_cli_pgn_bad_arguments(scamd):
    assert os.path.exists(PLAY)
    common = [PLAY, "--white-device", "cuda", "--black-type", "nn"]
    r = subprocess.run(common + ["--pgn"], capture_output=True, text=True)
    assert r.returncode == 2 and "missing value" in r.stderr
    r = subprocess.run(common + ["--pgn="], capture_output=True, text=True)
    assert r.returncode == 2 and "--pgn needs a file name" in r.stderr and "usage:" in r.stderr
    r = subprocess.run(common + ["--pgn", "--swap"], capture_output=True, text=True)
    assert r.returncode == 2 and "--pgn needs a file name" in r.stderr
    r = subprocess.run([PLAY, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--pgn FILE" in r.stderr
