"""Trace files written on the GPU (-m gpu): sc_traces_format against the pure-Python reference writer (tests/trace_write_ref.py,
itself held to the host writer by tests/test_trace_write_ref.py) on one hand-made batch that holds every edge -- child counts
around the 64-child rounds, games without steps, every outcome form, promotions, the count widths, the float edge set, "fen" and
"opening", ply offsets on every residue of the 16-byte store grid --, the buffer contract, the trace ring read in place against
the files the host writer writes for the same games, and the device reader on the device-written text.  ctypes only."""
import json

import numpy as np
import pytest

import trace_write_ref as ref
from support import FILL, _p, scamd_gpu, untouched  # noqa: F401

pytestmark = pytest.mark.gpu
FEN = "r1bqkbnr/pppp1ppp/2n5/4p3/4P3/5N2/PPPP1PPP/RNBQKB1R w KQkq - 2 3"
COUNTS = [0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999, 100000000, 999999999,
          1000000000, 2147483647]
OUTCOMES = [None, {"termination": "Checkmate", "winner": "White"}, {"termination": "Checkmate", "winner": "Black"},
            {"termination": "Stalemate", "winner": None}, {"termination": "InsufficientMaterial", "winner": None},
            {"termination": "SeventyfiveMoves", "winner": None}, {"termination": "FivefoldRepetition", "winner": None},
            {"termination": "FiftyMoves", "winner": None}, {"termination": "ThreefoldRepetition", "winner": None}]
MOVES = ["e2e4", "a7a8q", "h2h1n", "b7a8r", "c2d1b", "a1h8", "h8a1", "g1f3"]


@pytest.fixture(scope="module")
def traces(scamd):
    import scamd.traces as m
    return m


def _batch():
    """the hand-made batch and its reference texts.  The edge floats (about 1 300 patterns, one sign each, alternating) are dealt
    out as Q and uct of the children and as the steps' root values; the first step of every game with steps takes a root value
    of another length, chosen so that the ply offsets of the batch cover all 16 residues of the store grid"""
    vals = [float(v) for v in ref.f32(ref.edge_bits(signs=(0,)))]
    vals = [-v if i & 1 else v for i, v in enumerate(vals)]
    it = iter(range(10 ** 9))
    nxt = lambda: vals[next(it) % len(vals)]
    kid = lambda i: (MOVES[i % len(MOVES)], COUNTS[i % len(COUNTS)], nxt(), nxt())
    widths = [0, 1, 63, 64, 65, 128, 223, 224]
    games = []
    for g, oc in enumerate(OUTCOMES):
        if g in (1, 4, 8):
            games.append({"steps": [], "outcome": oc})    # no steps, between games with steps
            continue
        steps = [(MOVES[(g + i) % len(MOVES)], nxt(), [kid(g + i + k) for k in range(widths[(g + i) % len(widths)])]) for i in range(8 if g != 5 else 1)]
        games.append({"steps": steps, "outcome": oc})
    games[2]["opening"] = ["e2e4", "e7e5", "a7a8q"]
    games[3]["fen"] = FEN
    games[6]["fen"], games[6]["opening"] = FEN, ["g1f3"]
    games[8]["opening"] = ["d2d4"]
    assert len(vals) > 1300 and next(it) > len(vals)     # every edge float was used
    # first-step values of varying text length until the plies start on every residue
    fill = [1.0, 0.5, 0.25, 0.125, 1.0625, 1.03125, 1.015625, 1.0078125, 1.00390625, 1.001953125, 1.0009765625, 1.00048828125, 1.000244140625,
            1.0001220703125, 1.00006103515625, 1.000030517578125]
    for k in range(len(fill) ** 2):
        texts = [ref.trace_text(t) for t in games]
        residues, base = set(), 0
        for t, text in zip(games, texts):
            at = text.index(b'"steps": ') + 9 + 2
            for i in range(len(t["steps"])):
                residues.add((base + at) % 16)
                at = text.index(b"\n    ]", at) + 6 + (2 if i + 1 < len(t["steps"]) else 1)
            base += len(text)
        if len(residues) == 16:
            break
        g = (0, 2, 3, 6, 7)[k % 5]
        s = games[g]["steps"][0]
        games[g]["steps"][0] = (s[0], fill[(k // 5) % len(fill)], s[2])
    assert len(residues) == 16, sorted(residues)
    return games, texts


@pytest.fixture(scope="module")
def batch():
    return _batch()


def test_hand_made_batch_in_one_call(traces, batch):
    games, texts = batch
    assert sorted({len(s[2]) for t in games for s in t["steps"]}) == [0, 1, 63, 64, 65, 128, 223, 224]
    got = traces.format(games)
    for g, (a, b) in enumerate(zip(got, texts)):
        if a != b:
            k = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
            pytest.fail(f"game {g}: lengths {len(a)} / {len(b)}, first difference at byte {k}: {a[max(k - 40, 0):k + 40]!r} / {b[max(k - 40, 0):k + 40]!r}")
    assert [json.loads(t)["steps"][0][0] for t in got if json.loads(t)["steps"]] == [t["steps"][0][0] for t in games if t["steps"]]
    count_ms, emit_ms = traces.format_last_timing()
    assert count_ms > 0 and emit_ms > 0


def _raw(scamd, traces, games, cap=None, extra=64):
    """sc_traces_format into a buffer of the needed size + `extra` bytes, pre-filled with FILL -> (rc, buffer, sizing offsets, offsets)"""
    L = scamd.lib()
    n = len(games)
    args, keep = traces.pack_traces(games)
    sized, off = np.zeros(n + 1, np.uint64), np.full(n + 1, 7, np.uint64)
    assert L.sc_traces_format(0, n, *args, None, 0, _p(sized)) == 0, L.sc_last_error().decode()
    buf = np.full(int(sized[n]) + extra, FILL, np.uint8)
    rc = L.sc_traces_format(0, n, *args, _p(buf), int(sized[n]) if cap is None else cap, _p(off))
    del keep
    return rc, buf, sized, off


def test_buffer_contract(scamd, traces, batch):
    games, texts = batch
    total = sum(len(t) for t in texts)
    rc, buf, sized, off = _raw(scamd, traces, games)
    assert rc == 0 and np.array_equal(sized, off) and int(off[-1]) == total
    assert np.array_equal(np.diff(off.astype(np.int64)), [len(t) for t in texts])
    assert buf[:total].tobytes() == b"".join(texts) and untouched(buf[total:])
    rc, buf, _, _ = _raw(scamd, traces, games, cap=total - 1)
    assert rc == -1 and "cap" in scamd.lib().sc_last_error().decode() and untouched(buf)
    rc, buf, sized, off = _raw(scamd, traces, [])
    assert rc == 0 and int(sized[0]) == 0 and int(off[0]) == 0 and untouched(buf)
    assert traces.format([]) == []
    one = traces.format([{"steps": [], "outcome": None}])
    assert one == [b'{\n  "outcome": null,\n  "steps": []\n}']


def test_round_trip_through_the_device_reader(traces, batch):
    games, _ = batch
    t = traces.read(traces.format(games)).check()
    try:
        assert t.games() == [[(s[0], [(c[0], c[1]) for c in s[2]]) for s in g["steps"]] for g in games]
        assert t.openings() == [list(g.get("opening") or []) for g in games] and t.fens() == [g.get("fen") for g in games]
        want = [(0, 0, -1) if g["outcome"] is None else
                (1, traces.TERMINATION_NAMES.index(g["outcome"]["termination"]), {"White": 1, "Black": 0, None: -1}[g["outcome"]["winner"]]) for g in games]
        assert [tuple(int(x) for x in row) for row in zip(t.has_outcome, t.termination, t.winner)] == want
    finally:
        t.close()


def _file(sp, g, tmp_path):
    p = str(tmp_path / f"host_{g}.json")
    sp.write_trace(g, p)
    with open(p, "rb") as f:
        return f.read()


def test_ring_source(scamd, tmp_path):
    """12 games through a held ring of 8 rows: the text of every reported game equals the host writer's file, from memory and
    from write_traces' files, while the next steps are queued; codes 1 and 2"""
    sp = scamd.SelfPlay(None, n_slots=8, n_games=12, rollout_num=16, num_steps=10, evaluator="synth", trace_capacity=8, trace_hold=True,
                        temperature=1.0, temperature_switch=6, seed=5)
    try:
        with pytest.raises(scamd.EngineError) as e:
            sp.traces_json([11])
        assert e.value.code == 1
        first, released_checked, done = None, False, []
        for _ in range(400):
            sp.enqueue(16)
            fin = sp.poll()
            if first is not None and not released_checked:
                with pytest.raises(scamd.EngineError) as e:
                    sp.traces_json(first + fin)      # released by this poll: 2 wins
                assert e.value.code == 2
                with pytest.raises(scamd.EngineError) as e:
                    sp.write_traces(first, [str(tmp_path / "gone.json")] * len(first))
                assert e.value.code == 2 and not (tmp_path / "gone.json").exists()
                released_checked = True
            if fin:
                sp.enqueue(16)   # the held rows are final: formatted while these steps are queued
                got = sp.traces_json(fin)
                paths = [str(tmp_path / f"dev_{g}.json") for g in fin]
                sp.write_traces(fin, paths)
                for g, text, p in zip(fin, got, paths):
                    want = _file(sp, g, tmp_path)
                    assert text == want and open(p, "rb").read() == want, g
                done += fin
                if first is None:
                    first = list(fin)
            if sp.stats()["games_active"] == 0 and not fin:
                break
        assert released_checked and sorted(done) == list(range(12))
        assert sp.traces_json([]) == [] and sp.stats()["error_flags"] == 0
    finally:
        sp.close()


def test_ring_source_with_fen_and_opening(scamd, tmp_path):
    sp = scamd.SelfPlay(None, evaluator="synth", seed=5, with_noise=False, outcome_gate=-1, tie_random=True, rollout_num=20, cpuct=1.5,
                        temperature=0.0, temperature_switch=0, n_slots=4, n_games=6, num_steps=6)
    try:
        sp.set_match(None, None, 11, 22, colours=1)
        sp.set_openings([(FEN, ["f1c4", "f8c5"]), ["e2e4"], []])
        sp.run()
        got = sp.traces_json(range(6))
        for g in range(6):
            assert got[g] == _file(sp, g, tmp_path), g
        assert b'"fen": "' + FEN.encode() in got[0] and b'"opening": [\n    "f1c4"' in got[1] and b'"opening"' in got[2] and b'"fen"' not in got[2]
        assert b'"opening"' not in got[4]
    finally:
        sp.close()


def test_one_launch_handle_keeps_stepping(scamd, tmp_path):
    """a network handle in the one-launch form (its workgroups wait for each other inside a launch): held rows are formatted
    while its next steps run, the files are the host writer's and no hand-off timed out"""
    eng = scamd.Engine(2, 128, seed=3)
    sp = scamd.SelfPlay(eng, n_slots=64, n_games=128, rollout_num=8, num_steps=4, trace_capacity=128, trace_hold=True, seed=2)
    try:
        assert sp.launches_per_step() == 1
        done = []
        for _ in range(200):
            sp.enqueue(8)
            fin = sp.poll()
            if fin:
                sp.enqueue(16)
                got = sp.traces_json(fin)
                for g, text in zip(fin, got):
                    assert text == _file(sp, g, tmp_path), g
                done += fin
            if sp.stats()["games_active"] == 0 and not fin:
                break
        st = sp.stats()
        assert sorted(done) == list(range(128)) and st["error_flags"] == 0 and st["games_finished"] == 128
    finally:
        sp.close()
        eng.close()
