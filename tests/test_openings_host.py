"""Match play from opening lines, the checks that need no GPU: the opening-file parser, the line-assignment rule, and the two entry
points in the header, the library, the ctypes table and integration/hip.rs."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from support import ROOT, scamd_built  # noqa: F401

NEW = {"sc_selfplay_set_openings": 5, "sc_selfplay_get_opening": 4}


def test_read_openings_comments_blank_line_bad_token(scamd, tmp_path):
    from scamd.selfplay import read_openings
    p = tmp_path / "lines.txt"
    p.write_text("# a suite of four\n"
                 "e2e4 e7e5   g1f3 # the open game\n"
                 "\n"
                 "   # an indented comment is no opening either\n"
                 "a7a8q\tb2b1n\n"
                 "d2d4\n")
    assert read_openings(str(p)) == [["e2e4", "e7e5", "g1f3"], [], ["a7a8q", "b2b1n"], ["d2d4"]]
    p.write_text("e2e4 e7e5\nd2d4 Nf6\n")
    with pytest.raises(ValueError, match=r"lines\.txt:2: 'Nf6'"):
        read_openings(str(p))
    for bad in ("e2e9", "e2e4k", "e2", "i2i4"):
        p.write_text(bad + "\n")
        with pytest.raises(ValueError, match="not a UCI move"):
            read_openings(str(p))
    p.write_text("")
    assert read_openings(str(p)) == []


def test_opening_of_game_is_the_rule(scamd):
    from scamd.selfplay import opening_of_game
    for n_lines in (1, 2, 3, 7):
        for k in range(40):
            assert opening_of_game(k, n_lines, 0) == k % n_lines
            assert opening_of_game(k, n_lines, 1) == (k >> 1) % n_lines
    # alternating colours: the two games of a pair share their line, and the first 2 * n_lines games play every line twice
    assert [opening_of_game(k, 3, 1) for k in range(8)] == [0, 0, 1, 1, 2, 2, 0, 0]
    assert [opening_of_game(k, 3, 0) for k in range(8)] == [0, 1, 2, 0, 1, 2, 0, 1]


def test_entry_points_in_header_library_and_bindings(scamd):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sc_engine.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "integration", "hip.rs")).read()
    ext = re.sub(r"//.*", "", re.search(r'extern "C" \{(.*?)\n\}', rs, flags=re.S).group(1))
    L = scamd.lib()
    for name, n_args in NEW.items():
        m = re.search(rf"\bint\s+{name}\s*\((.*?)\)\s*;", hdr, flags=re.S)
        assert m and len(m.group(1).split(",")) == n_args, name
        assert hasattr(L, name), name
        res, args = scamd.binding.ABI[name]
        assert res is C.c_int and len(args) == n_args, name
        r = re.search(rf"fn {name}\((.*?)\)\s*->\s*c_int", ext, flags=re.S)
        assert r and len([a for a in r.group(1).split(",") if a.strip()]) == n_args, name
    assert callable(scamd.SelfPlay.set_openings) and callable(scamd.SelfPlay.get_opening)
    # the property the GPU tests use is stated where users read it
    text = open(os.path.join(ROOT, "include", "sc_engine.h")).read()
    assert "CONTINUATION of the from-the-start game of the same id" in text


def test_null_handle_is_refused(scamd):
    L = scamd.lib()
    moves, off, status = np.zeros(1, np.uint16), np.zeros(2, np.uint32), np.zeros(1, np.int32)
    rc = L.sc_selfplay_set_openings(None, 1, moves.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p))
    assert rc == -1 and "null handle" in L.sc_last_error().decode()
    assert L.sc_selfplay_get_opening(None, 0, None, 0) == -1
