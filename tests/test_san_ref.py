"""san_ref.py, the CPU yardstick of the SAN tests, checked on the CPU: its renderer against the words of the reference's own
games, and every word of its three styles against helpers.san_to_move."""
import os
import sys
from collections import Counter

import pytest

import helpers as H
from san_ref import PINNED_RIVAL, cpu_game, san_of, yardstick_moves
from support import GOLD, ROOT


@pytest.fixture(scope="module")
def reference_games():
    """the words of the 60 games of the reference's sample.csv (scamd.san's reader is plain Python: no library is loaded)"""
    sys.path.insert(0, os.path.join(ROOT, "smart-chess-rust_amd"))
    import scamd.san as san
    texts, _ = san.read_games_csv(os.path.join(GOLD, "ref_sample_games.csv"))
    return [t.split() for t in texts]


def test_renderer_reproduces_the_reference_games(orc, reference_games):
    seen = Counter()
    assert len(reference_games) == 60 and sum(len(g) for g in reference_games) == 3539
    for words in reference_games:
        assert cpu_game(orc, yardstick_moves(orc, " ".join(words)), seen=seen) == words
    assert seen["ep"] == 1 and seen["pinned_rival"] == 1 and seen["file_dis"] >= 1 and seen["rank_dis"] >= 1, dict(seen)


@pytest.mark.parametrize("style", ["min", "over", "noeq"])
def test_every_word_is_read_back_to_its_move(orc, style):
    """helpers.san_to_move reads "min" whole.  Of "over" it reads everything but castling spelt with the digit 0, which
    yardstick_moves maps to the letter O first; the same mapping is applied here.  Of "noeq" it reads every word but a promotion
    (it finds the promotion piece behind "="): those words are counted and skipped."""
    lines = [ln["uci"] for ln in H.load_edge_lines()] + [PINNED_RIVAL]
    seen = Counter()
    read = skipped = 0
    for uci in lines:
        st = orc.State()
        for u in uci:
            m = orc.from_uci(u)
            w = san_of(st, m, style, seen)
            if style == "noeq" and H.mv_parts(m)[2]:
                skipped += 1
            else:
                got, check, mate = H.san_to_move(st, w.replace("0", "O") if w.startswith("0-0") else w, orc)
                assert got == m and check == w.endswith(("+", "#")) and mate == w.endswith("#"), (st.fen(), w)
                read += 1
            st.push(m)
    assert read + skipped == 4408 + len(PINNED_RIVAL) and (skipped > 0) == (style == "noeq")
    for k in ("ep", "castle_k", "castle_q", "promo_capture_check", "underpromo") + (("file_dis", "rank_dis", "file_and_rank", "pinned_rival") if style != "over" else ()):
        assert seen[k] >= 1, (k, dict(seen))
