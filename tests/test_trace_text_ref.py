"""The reference reader of trace files (tests/trace_text_ref.py) on its own, no GPU: it gives back what the writer was given, and
it refuses every proper prefix of a file -- as json.loads does, so that the reference alone meets the condition the GPU test of
the truncation sweep imposes."""
import json
import os

import pytest
import trace_text_ref as ref
from support import GOLD, scamd_built  # noqa: F401


@pytest.fixture(scope="module")
def written(scamd, tmp_path_factory):
    """the golden trace excerpt and two hand-made traces, as sc_trace_write_json writes them: [(trace dict, file bytes)]"""
    fx = json.load(open(os.path.join(GOLD, "ref_fixtures.json")))
    steps = [(s[0], float(s[1]), [(c[0], c[1], float(c[2]), 0.5) for c in s[2]]) for s in fx["trace_first10"]]
    traces = [{"steps": steps, "outcome": fx["trace_outcome"]},
              {"steps": [("e7e8q", 1e-7, []), ("a2a1n", -0.0, [("h2h1r", 0, 1e20, 123456.5), ("a7a8b", 2147483647, float("nan"), 0.0)])], "outcome": None},
              {"steps": [], "outcome": {"termination": "Stalemate", "winner": None}}]
    out = []
    for i, tr in enumerate(traces):
        p = str(tmp_path_factory.mktemp("traces") / f"t{i}.json")
        scamd.write_trace_json(p, tr)
        out.append((tr, open(p, "rb").read()))
    return out


def test_reads_back_what_the_writer_was_given(scamd, written):
    for tr, text in written:
        r = ref.read_one(text)
        assert r["status"] == 0 and r["err_at"] == 0
        assert r["moves"] == [scamd.uci_move(s[0]) for s in tr["steps"]]
        assert r["children"] == [[(scamd.uci_move(c[0]), c[1]) for c in s[2]] for s in tr["steps"]]
        oc = tr["outcome"]
        want = (0, 0, -1) if oc is None else (1, ref.TERMINATION_NAMES.index(oc["termination"]), {"White": 1, "Black": 0, None: -1}[oc["winner"]])
        assert r["outcome"] == want and r["opening"] == [] and r["fen"] is None
    many = ref.read_many([t for _, t in written])
    assert many["move_off"].tolist() == [0, 10, 12, 12] and many["child_off"].size == 13 and many["status"].tolist() == [0, 0, 0]
    assert ref.uci_move(b"a7a8q") == scamd.uci_move("a7a8q") and ref.uci_move(b"e2e4") == scamd.uci_move("e2e4")


def test_every_proper_prefix_is_refused(written):
    text = written[1][1]
    assert 300 < len(text) < 1200 and text[-1:] == b"}"       # (no trailing white space: every proper prefix cuts a token)
    for k in range(len(text)):
        r = ref.read_one(text[:k])
        assert r["status"] < 0 and r["err_at"] <= k and not r["moves"], k
        with pytest.raises(ValueError):
            json.loads(text[:k].decode())
    assert ref.read_one(text)["status"] == 0


def test_single_defects_and_what_is_outside_the_contract():
    good = b'{"outcome": null, "steps": [["e2e4", 0.5, [["e2e4", 3, 0.1, null], ["d2d4", 0]]]]}'
    assert ref.read_one(good)["children"] == [[(ref.uci_move(b"e2e4"), 3), (ref.uci_move(b"d2d4"), 0)]]
    for text, code, at in ((good.replace(b'"d2d4"', b'"d2d9"'), ref.MOVE, good.index(b'"d2d4"')),
                           (good.replace(b" 3,", b" -3,"), ref.COUNT, good.index(b" 3,") + 1),
                           (good.replace(b"null,", b'"a\\n",'), ref.ESCAPE, good.index(b"null,") + 2),
                           (good.replace(b'"steps"', b'"stops"'), ref.STEPS, len(good)),
                           (good[:-1], ref.UNBALANCED, len(good) - 1), (b"", ref.UNBALANCED, 0)):
        r = ref.read_one(text)
        assert (r["status"], r["err_at"]) == (-code, at), text
    assert ref.read_one(good.replace(b"0.5, ", b""))["status"] == -ref.SHAPE
    assert ref.read_one(good.replace(b"null", b'{"winner": "Red", "termination": "Checkmate"}', 1))["status"] == -ref.OUTCOME
    for text in (good.replace(b"0.5", b"true"), b'{"steps": [1 2]}'):
        with pytest.raises(ValueError):
            ref.read_one(text)
