"""Device-resident training tensors on the GPU (-m gpu): sc_encode_steps_device and sc_selfplay_encode_traces next to the host
entry point (sc_encode_steps through encode_steps_batch), bit for bit.  The host entry point runs the same encoder into staging
buffers, so that comparison checks what differs between the entry points -- the host path's slices, staging and copy-out, stream
use, the ring as a source, the layouts, the grouping by history records -- and does not pin the kernels: the oracle does, on
sampled games of the device result (assert_games_equal_oracle) and of the host result.  Device buffers come from hipMalloc on
the HIP runtime libsc_engine.so uses (ctypes): this file does not import torch -- the torch interop runs in a child process of
its own."""
import os
import random

import numpy as np
import pytest

from helpers import random_games, random_steps
from support import ROOT, _p, _read, alloc_outputs, dev_per_test, run_steps, run_torch_child, scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu


def assert_games_equal_oracle(orc, r, steps, sample, mirror=False):
    """the games `sample` of r (a device result in the reference layout, or encode_steps_batch's) == orc.encode_steps, bit for bit"""
    off = r["ply_off"]
    for gi in sample:
        rc, b, m, d, idx = orc.encode_steps(steps[gi], mirror)
        a, e = int(off[gi]), int(off[gi + 1])
        assert rc == 0 and e - a == len(steps[gi])
        assert np.array_equal(r["boards"][a:e], b) and np.array_equal(r["meta"][a:e], m), gi
        assert np.array_equal(r["dist"][a:e].view(np.uint32), d.view(np.uint32)), gi
        for p in range(a, e):
            got = r["move_indices"][p] if "move_indices" in r else r["legal_idx"][p, :int(r["n_legal"][p])]
            assert np.array_equal(np.asarray(got, np.int32), idx[p - a]), (gi, p)


def assert_same_as_host(d, h, skip=None):
    """device result d (reference layout) == encode_steps_batch's h, bit for bit: the two entry points around the one encoder
    agree.  skip[g] = first failing ply of game g (outputs at and after it are unspecified, include/sc_engine.h)"""
    assert np.array_equal(d["status"], h["status"])
    off = h["ply_off"]
    keep = np.ones(int(off[-1]), bool)
    for g in range(len(off) - 1):
        if skip is not None and skip[g] is not None:
            keep[int(off[g]) + skip[g]:int(off[g + 1])] = False
    assert np.array_equal(d["boards"][keep], h["boards"][keep])
    assert np.array_equal(d["meta"][keep], h["meta"][keep])
    assert np.array_equal(d["dist"][keep].view(np.uint32), h["dist"][keep].view(np.uint32))
    for p in np.nonzero(keep)[0]:
        nl = int(d["n_legal"][p])
        assert np.array_equal(d["legal_idx"][p, :nl].astype(np.int32), h["move_indices"][p]), p
        assert not d["legal_idx"][p, nl:].any() and not d["dist_legal"][p, nl:].any(), p


def _first_bad_ply(status):
    return [None if s == 0 else (s - 1000 if s >= 1000 else -s - 1) for s in status.tolist()]


@pytest.mark.parametrize("mirror", [False, True])
def test_device_matches_host_path(scamd, orc, dev, mirror):
    rnd = random.Random(11)
    games = [g for g, _ in random_games(orc, 40, 120, seed=77) if g]
    games.append(games[0][:1])
    steps = [random_steps(orc, g, rnd) for g in games]
    steps.insert(3, [])   # a game without plies
    h = scamd.encode_steps_batch(steps, mirror)
    d = run_steps(scamd, dev, steps, mirror)
    assert (h["status"] == 0).all()
    assert_same_as_host(d, h)
    assert_games_equal_oracle(orc, d, steps, (0, len(steps) // 2, len(steps) - 1), mirror)


def test_device_errors_like_the_host_path(scamd, orc, dev):
    st = orc.State()
    good = [(m, 1) for m in st.legal_moves()]
    e2e4, e7e5 = orc.from_uci("e2e4"), orc.from_uci("e7e5")
    st.push(e2e4)
    good2 = [(m, 1) for m in st.legal_moves()]
    cases = [[(e2e4, good[:-1])], [(e2e4, good + [(e7e5, 1)])], [(e7e5, good)], [(e2e4, good), (e2e4, good2)],
             [(e2e4, good), (e7e5, good2[:-1] + [good2[0]])], [(e2e4, good), (e7e5, good2)]]
    h = scamd.encode_steps_batch(cases)
    assert h["status"].tolist() == [1000, 1000, -1, -2, 1001, 0]
    for mirror in (False, True):
        d = run_steps(scamd, dev, cases, mirror)
        assert_same_as_host(d, scamd.encode_steps_batch(cases, mirror), skip=_first_bad_ply(h["status"]))


def _long_and_short(orc):
    cyc = ["g1f3", "g8f6", "f3g1", "f6g8", "b1c3", "b8c6", "c3b1", "c6b8"]
    games = []
    for moves in ([cyc[i % 8] for i in range(700)], ["e2e4", "e7e5", "g1f3"]):
        st = orc.State()
        steps = []
        for m in moves:
            steps.append((m, [(orc.uci(x), 1 + (k % 3)) for k, x in enumerate(st.legal_moves())]))
            st.push(m)
        games.append(steps)
    return games


def _slices(ply_off, cap=8192):
    """the host path's slices (first game, one past the last): consecutive whole games of at most `cap` plies together"""
    out, g0, n = [], 0, len(ply_off) - 1
    while g0 < n:
        g1 = g0 + 1
        while g1 < n and int(ply_off[g1 + 1]) - int(ply_off[g0]) <= cap:
            g1 += 1
        out.append((g0, g1))
        g0 = g1
    return out


def test_long_game_among_many_short_ones(scamd, orc, dev):
    """a 700-ply game (repetition scan over > 64 plies) among 1 500 three-ply games: the game records exceed the per-call
    budget (1 501 x 702 > 2^20 records), so the games are encoded in groups -- results equal the host path"""
    games = _long_and_short(orc)
    batch = [games[1]] * 750 + [games[0]] + [games[1]] * 750
    h = scamd.encode_steps_batch(batch)
    d = run_steps(scamd, dev, batch)
    assert (d["status"] == 0).all()
    assert_same_as_host(d, h)
    assert_games_equal_oracle(orc, d, batch, (0, 750, 1500))
    p = int(h["ply_off"][750]) + 600
    assert d["boards"][p][:, :, 12].any() and d["boards"][p][:, :, 13].any()


def test_host_slices_and_record_groups_differ(scamd, orc):
    """the host path's slices (plies: staging) and the encoder's groups (history records) cut a batch in different places.
    One slice of several groups: the 700-ply game first, 1 500 three-ply games behind it.  Several slices of one group each:
    more than 8 192 plies with the 700-ply game in the middle.  The first and last game of every slice, the long game and a
    middle game equal the oracle"""
    long_game, short = _long_and_short(orc)
    batch = [long_game] + [short] * 1500
    r = scamd.encode_steps_batch(batch)
    assert (r["status"] == 0).all() and len(_slices(r["ply_off"])) == 1 and 1501 * 702 > 1 << 20
    assert_games_equal_oracle(orc, r, batch, (0, 1, 750, 1500))
    rnd = random.Random(2)
    base = [g for g, _ in random_games(orc, 30, 150, seed=5) if len(g) >= 40]
    steps = [random_steps(orc, g, rnd) for g in (base * 5)[:110]]
    steps.insert(55, long_game)
    r = scamd.encode_steps_batch(steps)
    sl = _slices(r["ply_off"])
    assert (r["status"] == 0).all() and int(r["ply_off"][-1]) > 8192 and len(sl) >= 2
    assert_games_equal_oracle(orc, r, steps, sorted({55, 20} | {g for a, b in sl for g in (a, b - 1)}))


def test_more_plies_than_one_host_chunk(scamd, orc, dev):
    rnd = random.Random(2)
    base = [g for g, _ in random_games(orc, 30, 150, seed=5) if len(g) >= 40]
    steps = [random_steps(orc, g, rnd) for g in (base * 5)[:110]]
    h = scamd.encode_steps_batch(steps)
    assert int(h["ply_off"][-1]) > 8192
    assert_same_as_host(run_steps(scamd, dev, steps), h)


def test_layouts_agree_and_sparse_equals_dense(scamd, orc, dev):
    rnd = random.Random(5)
    steps = [random_steps(orc, g, rnd) for g, _ in random_games(orc, 12, 90, seed=9) if g]
    for mirror in (False, True):
        ref = run_steps(scamd, dev, steps, mirror, layout=0)
        tr = run_steps(scamd, dev, steps, mirror, layout=1)
        assert np.array_equal(tr["boards"], ref["boards"].astype(np.float32).transpose(0, 3, 1, 2))
        assert np.array_equal(tr["meta"], ref["meta"].astype(np.float32))
        for k in ("dist", "dist_legal", "legal_idx", "n_legal", "status"):
            assert np.array_equal(tr[k], ref[k]), k
        # zeros(P, 4672).scatter_add_(1, legal_idx, dist_legal) == dist, bit for bit
        P = ref["dist"].shape[0]
        dense = np.zeros((P, 4672), np.float32)
        np.add.at(dense, (np.repeat(np.arange(P), 224), ref["legal_idx"].reshape(-1).astype(np.int64)), ref["dist_legal"].reshape(-1))
        assert np.array_equal(dense.view(np.uint32), ref["dist"].view(np.uint32))


def test_bad_pointers_are_refused(scamd, dev):
    games = [[("e2e4", [])]]
    mv, off, cm, cn, coff = scamd.pack_steps(games)
    L = scamd.lib()
    o = alloc_outputs(dev, 1, 1, 0)
    host = np.zeros(7168, np.int8)
    st_host = np.zeros(1, np.int32)
    rc = L.sc_encode_steps_device(None, 0, 1, _p(mv), _p(off), _p(cm), _p(cn), _p(coff), 0, 0, dev.stream, _p(host), None, None, None,
                                  None, None, o["status"])
    assert rc == -1 and "boards" in L.sc_last_error().decode() and "device memory" in L.sc_last_error().decode()
    rc = L.sc_encode_steps_device(None, 0, 1, _p(mv), _p(off), _p(cm), _p(cn), _p(coff), 0, 0, dev.stream, o["boards"], None, None,
                                  None, None, None, _p(st_host))
    assert rc == -1 and "status" in L.sc_last_error().decode()
    rc = L.sc_encode_steps_device(None, 0, 1, _p(mv), _p(off), _p(cm), _p(cn), _p(coff), 0, 2, dev.stream, o["boards"], None, None,
                                  None, None, None, o["status"])
    assert rc == -1 and "layout" in L.sc_last_error().decode()
    # ... and a good call on the same buffers still works afterwards (the failed pointer query left no sticky error)
    rc = L.sc_encode_steps_device(None, 0, 1, _p(mv), _p(off), _p(cm), _p(cn), _p(coff), 0, 0, dev.stream, o["boards"], None, None,
                                  None, None, None, o["status"])
    assert rc == 0
    dev.sync()
    assert dev.read(o["status"], (1,), np.int32).tolist() == [1000]   # no children recorded: "inconsistent moves" at ply 0


def _encode_traces(scamd, sp, dev, games, mirror=False, layout=0):
    L = scamd.lib()
    g = np.asarray(games, np.int32)
    off = np.zeros(len(games) + 1, np.uint32)
    rc = L.sc_selfplay_encode_traces(sp.h, len(games), _p(g), 0, 0, None, _p(off), None, None, None, None, None, None, None)
    if rc:
        return rc, None
    P = int(off[-1])
    o = alloc_outputs(dev, P, len(games), layout)
    rc = L.sc_selfplay_encode_traces(sp.h, len(games), _p(g), int(mirror), layout, dev.stream, _p(off), o["boards"], o["meta"], o["dist"],
                                     o["dist_legal"], o["legal_idx"], o["n_legal"], o["status"])
    assert rc == 0, L.sc_last_error().decode()
    dev.sync()
    r = _read(dev, o, P, len(games), layout)
    r["ply_off"] = off
    return 0, r


def test_trace_ring_in_place(scamd, dev):
    """a synthetic-evaluator handle with a trace ring and trace_hold, driven by enqueue + poll: games reported by poll are
    encoded from their held rows (after the next steps are enqueued) and equal get_trace + the host path; an unfinished game
    gives 1, a row released by the next poll gives 2"""
    sp = scamd.SelfPlay(None, n_slots=4, n_games=16, rollout_num=8, num_steps=14, evaluator="synth", trace_capacity=8,
                        trace_hold=True, temperature=1.0, temperature_switch=6, seed=5)
    try:
        rc, _ = _encode_traces(scamd, sp, dev, [15])
        assert rc == 1
        first, released_checked, n_checked = None, False, 0
        for _ in range(400):
            sp.enqueue(8)
            fin = sp.poll()
            if first is not None and not released_checked:
                rc, _ = _encode_traces(scamd, sp, dev, first)   # released by this poll
                assert rc == 2
                released_checked = True
            if fin:
                sp.enqueue(8)   # the held rows are final: encoded while these steps are queued
                for mirror in (False, True):
                    rc, d = _encode_traces(scamd, sp, dev, fin, mirror)
                    assert rc == 0
                    traces = [sp.trace(g) for g in fin]
                    steps = [[(s[0], [(c[0], c[1]) for c in s[2]]) for s in t["steps"]] for t in traces]
                    h = scamd.encode_steps_batch(steps, mirror)
                    assert (h["status"] == 0).all() and np.array_equal(d["ply_off"], h["ply_off"])
                    assert_same_as_host(d, h)
                n_checked += len(fin)
                if first is None:
                    first = list(fin)
            if sp.stats()["games_active"] == 0 and not fin:
                break
        assert released_checked and n_checked == 16
    finally:
        sp.close()


_CHILD = r'''
import json, os, sys
import torch                      # first: libsc_engine.so then binds to the runtime torch loaded
import torch.nn.functional as F
sys.path.insert(0, sys.argv[1])
import numpy as np
import scamd
out = {}
torch.zeros(1, device="cuda:0")
scamd.lib()
out["hip_runtimes"] = scamd.hip_runtime_files()
sp = scamd.SelfPlay(None, n_slots=8, n_games=8, rollout_num=8, num_steps=20, evaluator="synth", temperature=1.0,
                    temperature_switch=6, seed=3, outcome_gate=4)
sp.run()
traces = [sp.trace(g) for g in range(8)]
steps = [[(s[0], [(c[0], c[1]) for c in s[2]]) for s in t["steps"]] for t in traces]
win = [0.0 if t["outcome"] is None or t["outcome"]["winner"] is None else 1.0 if t["outcome"]["winner"] == "White" else -1.0
       for t in traces]
h = scamd.encode_steps_batch(steps, True)
r = scamd.encode_steps_torch(steps, apply_mirror=True, layout="reference", dist="both", outcomes=win)
ok = r["boards"].device == torch.device("cuda", 0) and (r["status"] == 0).all()
ok = ok and np.array_equal(r["boards"].cpu().numpy(), h["boards"]) and np.array_equal(r["meta"].cpu().numpy(), h["meta"])
ok = ok and np.array_equal(r["dist"].cpu().numpy().view(np.uint32), h["dist"].view(np.uint32))
dense = torch.zeros_like(r["dist"]).scatter_add_(1, r["legal_idx"].long(), r["dist_legal"])
ok = ok and torch.equal(dense, r["dist"])
out["host_equal"] = bool(ok)
t = scamd.encode_steps_torch(scamd.pack_steps(steps), apply_mirror=True, layout="trainer", dist="dense", outcomes=win)
out["trainer_equal"] = bool(torch.equal(t["boards"], r["boards"].float().permute(0, 3, 1, 2)) and torch.equal(t["meta"], r["meta"].float()))
exp_oc = -np.repeat(np.asarray(win, np.float32), np.diff(h["ply_off"].astype(np.int64)))
out["outcome_equal"] = bool(np.array_equal(t["outcome"].cpu().numpy(), exp_oc))
ring = sp.training_tensors(list(range(8)), apply_mirror=True, layout="trainer", dist="dense")
out["ring_equal"] = bool(torch.equal(ring["boards"], t["boards"]) and torch.equal(ring["meta"], t["meta"])
                         and torch.equal(ring["dist"], t["dist"]) and torch.equal(ring["outcome"], t["outcome"]))
sp.close()
# a trainer step on the tensors: policy cross-entropy with the visit distribution as target, value MSE on the outcome
torch.manual_seed(0)
net = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(112 * 64, 4672 + 1)).to("cuda:0")
y = net(t["boards"])
loss = F.cross_entropy(y[:, :4672], t["dist"]) + F.mse_loss(torch.tanh(y[:, 4672]), t["outcome"])
loss.backward()
out["loss"] = float(loss)
out["grad_finite"] = bool(all(torch.isfinite(p.grad).all() for p in net.parameters()))
torch.cuda.synchronize()
print(json.dumps(out))
'''


def test_torch_interop_in_a_fresh_process(scamd, tmp_path):
    """torch imported first, then scamd: one HIP runtime in the process, encode_steps_torch / training_tensors equal the host
    path on cuda:0, and a loss on them runs (a child process: this one keeps its own runtime)"""
    pytest.importorskip("torch")
    out = run_torch_child(tmp_path, _CHILD, os.path.join(ROOT, "smart-chess-rust_amd"), timeout=600)
    assert len(out["hip_runtimes"]) == 1, out
    assert out["host_equal"] and out["trainer_equal"] and out["outcome_equal"] and out["ring_equal"], out
    assert np.isfinite(out["loss"]) and out["grad_finite"], out
