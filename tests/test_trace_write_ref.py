"""The pure-Python reference of the trace writer (tests/trace_write_ref.py) held to today's host writer: trace_text against the
files scamd.write_trace_json writes (csrc/trace_json.hpp) on the golden excerpt and on hand-made traces, pretty against the
numbers in those files on the float edge set and 20 000 random patterns.  The host writer's C entry point takes no "fen" or
"opening"; those members are held to the text csrc/trace_json.hpp spells out, and on the GPU to the handle's own files
(tests/test_gpu_trace_write.py).  No GPU needed."""
import json
import os

import numpy as np
from support import GOLD, scamd_built  # noqa: F401

import trace_write_ref as ref


def _host_text(scamd, tmp_path, trace):
    p = str(tmp_path / "t.json")
    scamd.write_trace_json(p, trace)
    with open(p, "rb") as f:
        return f.read()


def test_trace_text_is_the_host_writers_on_the_golden_excerpt(scamd, tmp_path):
    fx = json.load(open(os.path.join(GOLD, "ref_fixtures.json")))
    steps = [(s[0], float(s[1]), [(c[0], c[1], float(c[2]), 0.5) for c in s[2]]) for s in fx["trace_first10"]]
    tr = {"steps": steps, "outcome": fx["trace_outcome"]}
    assert ref.trace_text(tr) == _host_text(scamd, tmp_path, tr)


def test_trace_text_is_the_host_writers_on_hand_made_traces(scamd, tmp_path):
    kid = lambda i: ("a7a8q" if i % 3 == 0 else "e2e4", i * 37, -1.5 / (i + 1), 0.25 * i)
    for tr in ({"steps": [], "outcome": None},
               {"steps": [], "outcome": {"termination": "Stalemate", "winner": None}},
               {"steps": [("e7e8q", 1e-7, []), ("a2a1n", -0.0, [("h2h1r", 0, 1e20, 123456.5)])], "outcome": None},
               {"steps": [("g1f3", float("nan"), [kid(i) for i in range(65)]), ("b8c6", float("-inf"), [kid(0)])],
                "outcome": {"termination": "Checkmate", "winner": "Black"}},
               {"steps": [("e2e4", 1e16, [("e7e5", 2147483647, 1e17, 1e-5)])], "outcome": {"termination": "FiftyMoves", "winner": "White"}}):
        assert ref.trace_text(tr) == _host_text(scamd, tmp_path, tr)


def test_fen_and_opening_members():
    tr = {"steps": [], "outcome": None, "fen": "8/8/8/8/8/8/4K3/4k3 w - - 0 1", "opening": ["e2e4", "a7a8q"]}
    assert ref.trace_text(tr) == (b'{\n  "outcome": null,\n  "steps": [],\n  "fen": "8/8/8/8/8/8/4K3/4k3 w - - 0 1",\n  "opening": [\n'
                                  b'    "e2e4",\n    "a7a8q"\n  ]\n}')
    assert json.loads(ref.trace_text(dict(tr, steps=[("e2e4", 0.5, [])])))["opening"] == ["e2e4", "a7a8q"]
    assert ref.trace_text({"steps": [], "outcome": None, "opening": []}) == b'{\n  "outcome": null,\n  "steps": []\n}'


def test_pretty_is_the_host_writers_number(scamd, tmp_path):
    """every number goes through the host writer as a step's Q: the file's tokens are fmt_f64's"""
    bits = np.concatenate([ref.edge_bits(), np.random.default_rng(11).integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32)])
    vals = ref.f32(bits)
    text = _host_text(scamd, tmp_path, {"steps": [("e2e4", float(v), []) for v in vals], "outcome": None}).decode()
    got = [ln.strip().rstrip(",") for ln in text.split("\n")[5::5]][:vals.size]
    want = [ref.pretty(v) for v in vals]
    assert len(got) == len(want) and got == want
    assert max(len(w) for w in want) <= 24
    assert ref.pretty(ref.f32(0xB77FFFFF)) == "-0.000015258788153005298"   # one below 2^-16
