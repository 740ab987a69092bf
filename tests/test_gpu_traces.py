"""Trace files read on the GPU (-m gpu): sc_traces_read against the pure-Python reference reader (tests/trace_text_ref.py) on the
smallest texts that can go wrong -- layout variants, chunk and load edges, more files than one scan tile, every refusal code, a
truncation sweep, long white-space runs -- and sc_traces_encode_device against the encoder on the Python-read games, bit for bit.
The parse tests use ctypes only; what needs torch runs in a child process of its own (torch first, then scamd)."""
import json
import os
import random
import re

import numpy as np
import pytest

import trace_text_ref as ref
from support import ROOT, run_torch_child, scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu
SUMMARY = ("status", "n_steps", "n_children", "n_opening", "has_fen")
FEN = "r1bqkbnr/pppp1ppp/2n5/4p3/4P3/5N2/PPPP1PPP/RNBQKB1R w KQkq - 2 3"


@pytest.fixture(scope="module")
def traces(scamd):
    import scamd.traces as m
    return m


def _mv(rng, promo=False):
    s = "abcdefgh"[rng.randrange(8)] + str(rng.randrange(1, 9)) + "abcdefgh"[rng.randrange(8)] + str(rng.randrange(1, 9))
    return s + (rng.choice("nbrq") if promo else "")


def synth(seed, plies=3, children=4, outcome=("Checkmate", "White"), **extra):
    """a trace dict of random (not legal: the parse does not care) moves in the file's shape, "outcome" first as the writer has it"""
    rng = random.Random(seed)
    steps = [[_mv(rng, i % 5 == 4), rng.random() * 20 - 10, [[_mv(rng, k % 7 == 6), rng.randrange(0, 500), rng.random(), rng.random()]
                                                              for k in range(children if isinstance(children, int) else children[i])]]
             for i in range(plies)]
    d = {}
    if outcome != "absent":
        d["outcome"] = None if outcome is None else {"termination": outcome[0], "winner": outcome[1]}
    d["steps"] = steps
    d.update(extra)
    return d


def dumps(d, **kw):
    return json.dumps(d, **kw).encode()


def same(traces, blobs, check_err=False):
    """one call on blobs: every summary field and every packed array equals the reference's; -> (Traces' summary dict, reference)"""
    want = ref.read_many(blobs)
    t = traces.read(blobs)
    try:
        assert len(t) == len(blobs)
        for k in SUMMARY:
            assert np.array_equal(getattr(t, k), want[k]), (k, np.nonzero(getattr(t, k) != want[k])[0][:8], getattr(t, k)[:8], want[k][:8])
        assert np.array_equal(np.stack([t.has_outcome, t.termination, t.winner], 1), want["outcome"])
        if check_err:
            assert np.array_equal(t.err_at, want["err_at"]), (t.err_at, want["err_at"])
        assert (t.err_at <= np.array([len(b) for b in blobs])).all() and (t.err_at[t.status == 0] == 0).all()
        mv, off = t.moves()
        cm, cn, coff = t.children()
        assert np.array_equal(off, want["move_off"]) and np.array_equal(mv, want["moves"])
        assert np.array_equal(coff, want["child_off"]) and np.array_equal(cm, want["child_mv"]) and np.array_equal(cn, want["child_n"])
        ops = t.openings()
        assert [len(o) for o in ops] == want["n_opening"].tolist()
        assert [m for o in ops for m in o] == [ref_uci(m) for m in want["opening"]]
        assert t.fens() == want["fens"]
        got = dict(status=t.status.copy(), err_at=t.err_at.copy(), n_steps=t.n_steps.copy())
    finally:
        t.close()
    return got, want


def ref_uci(m):
    m = int(m)
    return "abcdefgh"[m & 7] + str(((m >> 3) & 7) + 1) + "abcdefgh"[(m >> 6) & 7] + str(((m >> 9) & 7) + 1) + " pnbrq"[m >> 12].strip()


def variants(scamd, tmp_path):
    base = synth(1)
    p = str(tmp_path / "w.json")
    scamd.write_trace_json(p, {"steps": [(s[0], s[1], [tuple(c) for c in s[2]]) for s in base["steps"]], "outcome": base["outcome"]})
    blobs = [open(p, "rb").read(),                                   # the writer's pretty form
             dumps(base, indent=2), dumps(base, indent=1), dumps(base, separators=(",", ":")), dumps(base, indent="\t"),
             dumps(base, indent=2).replace(b"\n", b"\r\n"),
             dumps({"steps": base["steps"], "outcome": base["outcome"]}, indent=2),         # "steps" before "outcome"
             dumps({"note": "a [ b", **base, "tail": "} ] \"".replace('"', "'")}), dumps({**base, "x": [[["e2e4"]]], "y": {"steps": [["e2e4", 0, []]]}}),
             dumps({"x": [[["e2e4", 5]]], **base}, separators=(",", ":")), dumps({**base, "name": "König ♔"}, ensure_ascii=False),
             dumps(synth(2, plies=0)), dumps(synth(3, plies=3, children=[0, 1, 224])), dumps(synth(4, plies=1, children=224), indent=2)]
    counts = synth(5, plies=2, children=3)
    counts["steps"][0][0], counts["steps"][1][0] = "a7a8q", "h2h1r"
    counts["steps"][0][2][0][1], counts["steps"][0][2][1][1] = 0, 4294967295
    counts["steps"][0][1] = None
    counts["steps"][1][2][0][2:] = [None, None]
    counts["steps"][1][2][1] = counts["steps"][1][2][1][:2]          # a child of move and count alone
    blobs += [dumps(counts), dumps(counts, indent=2), dumps(synth(6, outcome=None)), dumps(synth(7, outcome=("Stalemate", None)), indent=2),
              dumps(synth(8, outcome="absent")), dumps(synth(9, outcome=("Checkmate", "Black")), separators=(",", ":"))]
    blobs += [dumps(synth(20 + i, plies=1, children=2, outcome=(name, (None, "White", "Black")[i % 3])), indent=(None, 2)[i % 2])
              for i, name in enumerate(ref.TERMINATION_NAMES[1:])]
    blobs += [dumps(synth(40, opening=["e2e4", "e7e5", "g1f3"]), indent=2), dumps(synth(41, fen=FEN, opening=["f1b5"])), dumps(synth(42, fen=FEN), indent=2),
              dumps({"fen": FEN, "opening": [], **synth(43)}, separators=(",", ":")), dumps({"opening": ["a7a8n"], **synth(44, plies=0)})]
    swapped = {"outcome": {"winner": "Black", "termination": "FiftyMoves"}, "steps": base["steps"]}
    blobs += [dumps(base, indent=4), dumps(base, indent=2) + b"\n", dumps(swapped, indent=2), dumps(base, separators=(" , ", " : ")),
              dumps(synth(10, plies=5, children=30), indent=2)]
    return blobs


def test_equals_the_reference_reader(scamd, traces, tmp_path):
    blobs = variants(scamd, tmp_path)
    assert len(blobs) >= 38
    got, want = same(traces, blobs)
    assert (got["status"] == 0).all() and want["n_steps"].sum() > 50 and want["n_children"].max() == 225
    assert want["has_fen"].sum() == 3 and want["n_opening"].sum() == 5 and sorted(set(want["outcome"][:, 1])) == list(range(0, 11))


def _pad_to(blob, size):
    """blob (indent=2 form) grown to exactly `size` bytes by spaces behind its line ends, at most 200 per run"""
    lines = blob.split(b"\n")
    need = size - len(blob)
    assert 0 <= need <= 200 * (len(lines) - 1)
    out = []
    for ln in lines[:-1]:
        k = min(need, 200)
        need -= k
        out.append(ln + b"\n" + b" " * k)
    res = b"".join(out) + lines[-1]
    assert len(res) == size
    return res


def test_chunk_and_load_edges(traces):
    one = dumps(synth(50, plies=9, children=11, opening=["e2e4"], fen=FEN), indent=2)
    assert 8192 < len(one) < 16384          # three chunks: with 17 shifts every token kind crosses a 4 096 and a 16-byte edge
    blobs = [b" " * k + one for k in range(0, 4113, 257)]        # 0 .. 4 112 bytes in front
    assert len(blobs) == 17
    small = dumps(synth(51, plies=3, children=5), indent=2)
    mid = dumps(synth(52, plies=6, children=6), indent=2)
    assert len(small) < 4096 - 100 and 4096 < len(mid) < 8192 - 100
    blobs += [_pad_to(small, 4096), _pad_to(mid, 8192), dumps(synth(53, plies=300, children=28), indent=2), b'{"steps":[]}', b"{}", b""]
    assert len(blobs[19]) > 250 * 4096 * 0.9 and len(blobs[20]) < 16
    got, want = same(traces, blobs)
    assert got["status"].tolist() == [0] * 21 + [-ref.STEPS, -ref.UNBALANCED] and got["n_steps"][19] == 300
    for k in range(1, 17):                  # the same trace at every shift
        assert want["n_steps"][k] == want["n_steps"][0]


def test_more_files_than_one_scan_tile(traces):
    blobs = [dumps(synth(100 + i, plies=2, children=1 + i % 3), separators=(",", ":")) for i in range(1100)]
    for i in (0, 1023, 1024, 1099):
        blobs[i] = blobs[i].replace(b'"steps"', b'"stops"')
    got, want = same(traces, blobs, check_err=True)
    assert (np.nonzero(got["status"])[0] == [0, 1023, 1024, 1099]).all() and (got["status"][[0, 1023, 1024, 1099]] == -ref.STEPS).all()
    assert want["move_off"][-1] == 2 * 1096 and want["child_off"][-1] == want["n_children"].sum()


def _defects():
    """(file bytes, code, err_at or None) of single-defect files: every row of the header's table"""
    good = dumps(synth(60, plies=2, children=2, opening=["e2e4"]), indent=2)
    g2 = json.loads(good)
    in_string = good.index(b'"', good.index(b'"steps"') + 8) + 3      # inside the first step's move

    def with_step_move(m):
        d = json.loads(good)
        d["steps"][1][0] = m
        return dumps(d, indent=2)

    def with_count(tok):
        d = json.loads(good)
        d["steps"][0][2][1][1] = "@@"
        return dumps(d, indent=2).replace(b'"@@"', tok)

    out = [(good[:-1], ref.UNBALANCED, len(good) - 1), (good[:in_string], ref.UNBALANCED, in_string), (good + b"]", ref.UNBALANCED, len(good)),
           (b"[" + good[1:], ref.UNBALANCED, 0), (b"", ref.UNBALANCED, 0), (b"  \n", ref.UNBALANCED, 3)]
    esc = dumps({**g2, "note": "a\\b"}, indent=2)
    out.append((esc, ref.ESCAPE, esc.index(b"\\")))
    out += [(good.replace(b'"steps"', b'"stops"'), ref.STEPS, len(good)), (dumps({**g2, "more": 1}).replace(b'"more": 1', b'"steps": []'), ref.STEPS, None),
            (dumps({**g2, "steps": 5}), ref.STEPS, None)]
    for steps in ([5], [["e2e4", 0.5]], [["e2e4", 0.5, [], []]], [[0.5, "e2e4", []]], [["e2e4", 0.5, [5]]], [["e2e4", 0.5, [[7, "e2e4"]]]],
                  [["e2e4", 0.5, [["e2e4"]]]], [[]], [["e2e4", [], 0.5]]):
        out.append((dumps({**g2, "steps": steps}), ref.SHAPE, None))
    for m in ("e2e9", "e2", "e2e4k", "E2E4"):
        b = with_step_move(m)
        out.append((b, ref.MOVE, b.index(b'"' + m.encode() + b'"')))
    b = dumps({**g2, "opening": ["e2e4", "i2e4"]})
    out.append((b, ref.MOVE, b.index(b'"i2e4"')))
    d = json.loads(good)
    d["steps"][1][2][0][0] = "a1a9"
    b = dumps(d, separators=(",", ":"))
    out.append((b, ref.MOVE, b.index(b'"a1a9"')))
    for tok in (b"-1", b"1.0", b"1e3", b"null", b"4294967296"):
        b = with_count(tok)
        out.append((b, ref.COUNT, b.index(b" " + tok + b",") + 1))
    out.append((dumps(synth(61, plies=2, children=[3, 225])), ref.CHILDREN, None))
    out.append((dumps(synth(62, plies=4001, children=0), separators=(",", ":")), ref.PLIES, None))
    for oc in (5, "Checkmate", {"termination": "Checkmate"}, {"termination": "Mate", "winner": "White"}, {"termination": "Checkmate", "winner": "Red"}, []):
        out.append((dumps({**g2, "outcome": oc}), ref.OUTCOME, None))
    return out


def test_every_refusal_code(traces):
    """each single-defect file sits between two good files whose arrays must not change"""
    defects = _defects()
    assert {c for _, c, _ in defects} == set(range(1, 10))
    good = [dumps(synth(70 + i, plies=2, children=3), indent=(None, 2)[i % 2]) for i in range(len(defects) + 1)]
    blobs = [good[0]]
    for (b, _, _), g in zip(defects, good[1:]):
        blobs += [b, g]
    got, want = same(traces, blobs)
    for i, (b, code, at) in enumerate(defects):
        assert got["status"][2 * i + 1] == -code, (i, b[:80], got["status"][2 * i + 1], code)
        if at is not None:
            assert got["err_at"][2 * i + 1] == at == want["err_at"][2 * i + 1], (i, b[:80], got["err_at"][2 * i + 1], at)
    assert (got["status"][0::2] == 0).all() and (got["n_steps"][0::2] == 2).all()


def test_truncation_sweep(traces):
    full = dumps(synth(80, plies=2, children=2, outcome=("FiftyMoves", None), opening=["e2e4"], fen=FEN), indent=1)
    assert 500 < len(full) < 800 and full[-1:] == b"}"
    blobs = [full[:k] for k in range(len(full))] + [full]
    t = traces.read(blobs)
    try:
        assert (t.status[:-1] < 0).all(), np.nonzero(t.status[:-1] >= 0)[0]
        assert t.status[-1] == 0 and (t.n_steps[:-1] == 0).all() and t.n_steps[-1] == 2 and (t.err_at[:-1] <= np.arange(len(full))).all()
        with pytest.raises(traces.EngineError, match="UNBALANCED at byte"):
            t.check()
    finally:
        t.close()


def test_white_space_runs(traces):
    base = dumps(synth(90, plies=2, children=2), indent=2)
    want = ref.read_many([base])

    def runs(k):   # a run of exactly k in front of a key, behind the '[' of "steps", behind a comma between children
        i0, i1 = base.index(b'"steps"'), base.index(b"[", base.index(b'"steps"')) + 1
        s = base[:i0].rstrip() + b" " * k + base[i0:i1] + b"\t" * k + base[i1:].lstrip()
        return re.sub(rb"\],\n *", b"]," + b"\n" * k, s, count=1)

    assert same(traces, [runs(255)])[0]["status"][0] == 0
    for k in (256, 5000):
        t = traces.read([base, runs(k), base])
        try:
            assert t.status[0] == 0 and t.status[2] == 0 and t.status[1] in (0, -ref.SPACE)
            mv, off = t.moves()
            n = 3 if t.status[1] == 0 else 2
            assert np.array_equal(mv, np.tile(want["moves"], n)) and np.array_equal(t.children()[1], np.tile(want["child_n"], n))
        finally:
            t.close()


def test_handles_come_and_go(traces):
    blobs = [dumps(synth(95 + i, plies=2, children=2)) for i in range(3)] + [b"{"]
    want = ref.read_many(blobs)
    for _ in range(50):
        t = traces.read(blobs)
        assert t.status.tolist() == [0, 0, 0, -ref.UNBALANCED]
        t.close()
    t = traces.read(blobs)
    assert np.array_equal(t.moves()[0], want["moves"]) and np.array_equal(t.children()[1], want["child_n"])
    t.close()
    t.close()                                    # (twice: a closed handle stays closed)
    e = traces.read([])
    assert len(e) == 0 and e.moves()[1].tolist() == [0] and e.games() == []
    e.close()
    test_chunk_and_load_edges(traces)            # another test's read still gives the same arrays


# ------------------------------------------------------------------ the encoder on parsed traces (torch: a child process)
_CHILD = r'''
import ctypes as C, json, os, sys
import torch                      # first: libsc_engine.so then binds to the runtime torch loaded
sys.path.insert(0, sys.argv[1])
import numpy as np
import scamd
import scamd.traces as traces
tmp = sys.argv[2]
out = {}
torch.zeros(1, device="cuda:0")
eng = scamd.Engine(2, 128, seed=1)
sp = scamd.SelfPlay(eng, n_slots=16, n_games=16, rollout_num=8, num_steps=40, cpuct=2.5, temperature=0.0, temperature_switch=8, epsilon=0.15,
                    with_noise=True, seed=5, outcome_gate=10 ** 6)
sp.run()
paths, py_games, outcomes = [], [], []
for g in range(16):
    p = os.path.join(tmp, "g%d.json" % g)
    sp.write_trace(g, p)
    paths.append(p)
    tr = sp.trace(g)
    py_games.append([(s[0], [(c[0], c[1]) for c in s[2]]) for s in tr["steps"]])
    oc = json.load(open(p))["outcome"]
    outcomes.append(0.0 if oc is None else {"White": 1.0, "Black": -1.0, None: 0.0}[oc["winner"]])
sp.close()
t = traces.read(paths[:8] + [open(p, "rb").read() for p in paths[8:]])
t.check(paths)
out["plies"] = int(t.n_steps.sum())
out["games_equal"] = t.games() == py_games and t.games(5, 7) == py_games[5:12]
out["outcomes_equal"] = t.outcomes.tolist() == outcomes
KEYS = ("boards", "meta", "dist", "dist_legal", "legal_idx", "n_legal", "outcome")
def equal(a, b, rows=None):
    for k in KEYS:
        x, y = a[k], b[k]
        if (x is None) != (y is None):
            return False
        if x is not None and not torch.equal(x, y if rows is None else y[rows[0]:rows[1]]):
            return False
    return True
ok, sub, stream_ok = True, True, True
for layout in ("reference", "trainer"):
    for dist in ("dense", "legal", "both"):
        for mirror in (False, True):
            a = traces.encode_traces_torch(t, apply_mirror=mirror, layout=layout, dist=dist, engine=eng if mirror else None)
            b = scamd.encode_steps_torch(py_games, apply_mirror=mirror, layout=layout, dist=dist, outcomes=outcomes)
            ok = ok and equal(a, b) and np.array_equal(a["status"], b["status"]) and not a["status"].any() and np.array_equal(a["ply_off"], b["ply_off"])
    c = traces.encode_traces_torch(t, g0=5, n=7, layout=layout, dist="both")
    p0, p1 = int(b["ply_off"][5]), int(b["ply_off"][12])
    b2 = scamd.encode_steps_torch(py_games, layout=layout, dist="both", outcomes=outcomes)
    sub = sub and equal(c, b2, (p0, p1)) and c["ply_off"].tolist() == (b2["ply_off"][5:13] - p0).tolist() and not c["status"].any()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = traces.encode_traces_torch(t, layout=layout, dist="both")
    s.synchronize()
    stream_ok = stream_ok and equal(d, b2)
out["tensors_equal"], out["sub_range_equal"], out["stream_equal"] = ok, sub, stream_ok
L = scamd.lib()
host = np.zeros(64, np.int32)
st = torch.zeros(16, dtype=torch.int32, device="cuda:0")
rc = L.sc_traces_encode_device(None, t.h, 0, 16, 0, 0, None, host.ctypes.data_as(C.c_void_p), None, None, None, None, None, C.c_void_p(st.data_ptr()))
out["host_pointer"] = [rc, "boards" in L.sc_last_error().decode()]
rc = L.sc_traces_encode_device(None, t.h, 0, 16, 0, 0, None, None, None, None, None, None, None, host.ctypes.data_as(C.c_void_p))
out["host_status"] = [rc, L.sc_traces_encode_device(None, t.h, 10, 7, 0, 0, None, None, None, None, None, None, None, C.c_void_p(st.data_ptr()))]
t.close()
# statuses: a refused file, a file with "opening", children that miss a legal move, a good game
good = py_games[3]
k = next(i for i, s in enumerate(good) if len(s[1]) > 1)
broken = [(s[0], s[1][:-1] if i == k else s[1]) for i, s in enumerate(good)]
def text(game, **extra):
    return json.dumps({"outcome": None, "steps": [[s[0], 0.5, [[c[0], c[1], 0.0, 0.0] for c in s[1]]] for s in game], **extra}, indent=2).encode()
t = traces.read([text(good)[:-1], text(good, opening=["e2e4"]), text(broken), text(good)])
a = traces.encode_traces_torch(t, layout="reference", dist="legal")
b = scamd.encode_steps_torch([[], good, broken, good], layout="reference", dist="legal")
out["statuses"] = [a["status"].tolist(), b["status"].tolist(), a["ply_off"].tolist(), k]
n = len(good)
out["good_unaffected"] = all(torch.equal(a[x][2 * n:3 * n], b[x][2 * n:3 * n]) for x in ("boards", "meta", "dist_legal", "legal_idx", "n_legal"))
t.close()
eng.close()
torch.cuda.synchronize()
print(json.dumps(out))
'''


def test_encoder_on_parsed_traces_in_a_fresh_process(scamd, tmp_path):
    """torch first, then scamd: 16 quick self-play games written with SelfPlay.write_trace and read back -- Traces.games() is
    SelfPlay.trace()'s moves and counts, encode_traces_torch is encode_steps_torch on the Python-read games in every tensor
    (both layouts, all three dist modes, mirror off and on, a sub-range, a non-default stream), a host pointer is refused, and
    the reader's statuses stand over the encoder's"""
    pytest.importorskip("torch")
    out = run_torch_child(tmp_path, _CHILD, os.path.join(ROOT, "smart-chess-rust_amd"), str(tmp_path), timeout=600)
    assert out["plies"] > 100 and out["games_equal"] and out["outcomes_equal"], out
    assert out["tensors_equal"] and out["sub_range_equal"] and out["stream_equal"], out
    assert out["host_pointer"] == [-1, True] and out["host_status"] == [-1, -1], out
    got, want, ply_off, k = out["statuses"]
    n = ply_off[2] - ply_off[1]
    assert got == [300000 + ref.UNBALANCED, 400000, 1000 + k, 0] and want[2] == 1000 + k and want[3] == 0, out
    assert ply_off == [0, 0, n, 2 * n, 3 * n] and out["good_unaffected"], out
