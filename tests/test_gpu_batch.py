"""Shuffled training minibatches on the GPU (-m gpu): sc_gather_batch against the numpy yardstick (tests/batch_ref.py) on synthetic
sources and against the trainer-layout tensors the encoder itself writes, bit for bit -- there is no tolerance in this feature;
bad input is contained on the device; bad pointers are refused; and the replay buffer on top of it, in a child process that
imports torch before scamd.  Device buffers come from hipMalloc on the HIP runtime libsc_engine.so uses (ctypes): this file does
not import torch."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import batch_ref
from helpers import bits, random_games, random_steps
from support import FILL, ROOT, _p, alloc_outputs, open_dev, run_torch_child, scamd_gpu, untouched  # noqa: F401

pytestmark = pytest.mark.gpu
N_LEGAL = (0, 1, 63, 64, 65, 128, 129, 192, 193, 218)   # the boundaries of the scatter's lane rounds
KEYS = ("boards", "meta", "dist_legal", "legal_idx", "n_legal", "outcome")


@pytest.fixture(scope="module")
def dev(scamd):
    yield from open_dev(scamd, FILL)


def synthetic_source(n_src=37, seed=1):
    """random int8 planes (negatives, -128 and 127 included) and meta; n_legal over the lane-round boundaries; distinct random
    action indices per row with action 0, 4671 and the last 16-byte chunk 4668..4671 among them; shares with zeros among them;
    garbage past n_legal -- NaN shares and action indices up to 65535 -- that must not be looked at"""
    rng = np.random.default_rng(seed)
    b = rng.integers(-128, 128, (n_src, 8, 8, 112)).astype(np.int8)
    b[0, 0, 0, :4] = [-128, 127, -1, 1]
    m = rng.integers(-5, 400, (n_src, 7)).astype(np.int32)
    m[:, 0] = rng.integers(0, 2, n_src)
    li = rng.integers(0, 65536, (n_src, 224)).astype(np.uint16)
    dl = np.full((n_src, 224), np.nan, np.float32)
    dl[::2] = rng.standard_normal((len(dl[::2]), 224)).astype(np.float32) * 1e30
    nl = np.array([N_LEGAL[i % len(N_LEGAL)] for i in range(n_src)], np.int32)
    for r in range(n_src):
        n = int(nl[r])
        acts = rng.choice(np.arange(1, 4668), n, replace=False)
        if n >= 1 and r % 3 == 1:
            acts[rng.integers(0, n)] = 0
        if n >= 63 and r % 2 == 0:
            acts[rng.choice(n, 4, replace=False)] = [4668, 4669, 4670, 4671]
        elif n >= 1 and r % 5 == 1:
            acts[n - 1] = 4671
        sh = rng.random(n).astype(np.float32)
        sh[rng.random(n) < 0.2] = 0.0
        li[r, :n] = acts
        dl[r, :n] = sh
    oc = rng.integers(-1, 2, n_src).astype(np.float32)
    src = dict(boards=b, meta=m, dist_legal=dl, legal_idx=li, n_legal=nl, outcome=oc)
    used = [set(li[r, :nl[r]].tolist()) for r in range(n_src)]
    assert any(0 in u for u in used) and any({4668, 4669, 4670, 4671} <= u for u in used) and any(4671 in u and 4670 not in u for u in used)
    assert all(len(u) == nl[r] for r, u in enumerate(used)) and (b < 0).any()
    return src


@pytest.fixture(scope="module")
def source(dev):
    src = synthetic_source()
    return src, {k: dev.upload(src[k]) for k in KEYS}


def run_gather(scamd, dev, d_src, n_src, rows, mirror=None, want=(True, True, True, True), n_batch=None, expect_rc=0):
    """sc_gather_batch on the non-default stream into 0x5a-filled buffers -> what the buffers hold afterwards"""
    rows = np.asarray(rows, np.int32)
    B = len(rows)
    sizes = (B * 7168 * 4, B * 28, B * 4672 * 4, B * 4)
    outs = [dev.alloc(s) for s in sizes]
    n_bad = dev.alloc(4)
    d_rows = dev.upload(rows)
    d_mir = None if mirror is None else dev.upload(np.asarray(mirror, np.uint8))
    rc = scamd.lib().sc_gather_batch(0, n_src, B if n_batch is None else n_batch, d_rows, d_mir, *[d_src[k] for k in KEYS], dev.stream,
                                     *[o if w else None for o, w in zip(outs, want)], n_bad)
    assert rc == expect_rc, scamd.lib().sc_last_error().decode()
    dev.sync()
    shapes = ((B, 112, 8, 8), (B, 7), (B, 4672), (B,))
    got = [dev.read(o, s, np.float32) for o, s in zip(outs, shapes)]
    return got, int(dev.read(n_bad, (1,), np.int32)[0])


def assert_equal_ref(got, ref, what=""):
    for name, g, e in zip(("boards", "meta", "dist", "outcome"), got, ref):
        assert np.array_equal(bits(g), bits(e)), (what, name)


BATCHES = {
    "one": [36],
    "repeated": [3, 3, 0, 36, 3],
    "reversed": list(range(36, -1, -1)),
    "more_workgroups_than_rows": [(7 * i + 3) % 37 for i in range(131)],
}


def _mirror(kind, B):
    return None if kind == "none" else np.ones(B, np.uint8) if kind == "all" else (np.arange(B) % 3 != 1).astype(np.uint8) * 7


@pytest.mark.parametrize("mirror", ["none", "all", "mixed"])
@pytest.mark.parametrize("batch", list(BATCHES))
def test_synthetic_sources_bit_equal(scamd, dev, source, batch, mirror):
    src, d_src = source
    rows = BATCHES[batch]
    mir = _mirror(mirror, len(rows))
    got, n_bad = run_gather(scamd, dev, d_src, 37, rows, mir)
    ref = batch_ref.gather(src, rows, mir)
    assert ref[4] == 0 and n_bad == 0
    assert_equal_ref(got, ref[:4], batch)


def test_each_output_may_be_null_and_an_empty_batch_writes_nothing(scamd, dev, source):
    src, d_src = source
    rows = BATCHES["repeated"]
    mir = _mirror("mixed", len(rows))
    ref = batch_ref.gather(src, rows, mir)[:4]
    for skip in range(4):
        want = tuple(i != skip for i in range(4))
        got, n_bad = run_gather(scamd, dev, d_src, 37, rows, mir, want)
        assert n_bad == 0
        for i in range(4):
            if i == skip:
                assert untouched(got[i]), i
            else:
                assert np.array_equal(bits(got[i]), bits(ref[i])), (skip, i)
    # n_bad may be NULL too
    outs = [dev.alloc(len(rows) * n) for n in (7168 * 4, 28, 4672 * 4, 4)]
    rc = scamd.lib().sc_gather_batch(0, 37, len(rows), dev.upload(np.asarray(rows, np.int32)), None, *[d_src[k] for k in KEYS], dev.stream,
                                     *outs, None)
    assert rc == 0
    dev.sync()
    assert np.array_equal(bits(dev.read(outs[2], (len(rows), 4672), np.float32)), bits(batch_ref.gather(src, rows)[2]))
    # n_batch = 0: a successful no-op, n_bad included
    got, n_bad = run_gather(scamd, dev, d_src, 37, rows, mir, n_batch=0)
    assert all(untouched(g) for g in got) and n_bad == int.from_bytes(bytes([FILL] * 4), "little")


def test_bad_input_is_contained(scamd, dev, source):
    """one batch of 8: a row of -1, a row of n_src, a source row with n_legal = 219, one with an action index 4672 inside
    n_legal -- NaN as the header says, the other four samples bit-equal to the yardstick, n_bad = 4, twice the same bits"""
    src, _ = source
    src = {k: v.copy() for k, v in src.items()}
    n_src = 37
    r_nl, r_idx = 9, 5   # n_legal 218 / 128 in the synthetic source
    src["n_legal"][r_nl] = 219
    src["legal_idx"][r_idx, 100] = 4672
    assert src["n_legal"][r_idx] > 100
    d_src = {k: dev.upload(src[k]) for k in KEYS}
    rows = [2, -1, r_nl, 36, n_src, r_idx, 0, 11]
    mir = [1, 1, 0, 0, 1, 1, 0, 1]
    got, n_bad = run_gather(scamd, dev, d_src, n_src, rows, mir)
    ref = batch_ref.gather(src, rows, mir)
    assert ref[4] == 4 and n_bad == 4
    for b in (1, 4):
        assert all(np.isnan(g[b]).all() for g in got), b
    for b in (2, 5):
        assert np.isnan(got[2][b]).all() and not any(np.isnan(got[i][b]).any() for i in (0, 1, 3)), b
    good = [0, 3, 6, 7]
    for i, name in enumerate(("boards", "meta", "dist", "outcome")):
        keep = good if i == 2 else [0, 2, 3, 5, 6, 7]
        assert np.array_equal(bits(got[i][keep]), bits(ref[i][keep])), name
    again, n_bad2 = run_gather(scamd, dev, d_src, n_src, rows, mir)
    assert n_bad2 == 4
    assert_equal_ref(again, got, "second call")


def test_bad_pointers_are_refused(scamd, dev, source):
    src, d_src = source
    L = scamd.lib()
    rows = np.zeros(1, np.int32)
    d_rows = dev.upload(rows)
    out = dev.alloc(7168 * 4)
    host_out = np.zeros(7168, np.float32)
    srcs = [d_src[k] for k in KEYS]
    rc = L.sc_gather_batch(0, 37, 1, _p(rows), None, *srcs, dev.stream, out, None, None, None, None)
    assert rc == -1 and "rows" in L.sc_last_error().decode() and "device memory" in L.sc_last_error().decode()
    rc = L.sc_gather_batch(0, 37, 1, d_rows, None, _p(src["boards"]), *srcs[1:], dev.stream, out, None, None, None, None)
    assert rc == -1 and "boards" in L.sc_last_error().decode()
    rc = L.sc_gather_batch(0, 37, 1, d_rows, None, *srcs, dev.stream, _p(host_out), None, None, None, None)
    assert rc == -1 and "out_boards" in L.sc_last_error().decode()
    rc = L.sc_gather_batch(0, 37, 1, d_rows, None, *srcs, dev.stream, C.c_void_p(out.value + 4), None, None, None, None)
    assert rc == -1 and "16-byte" in L.sc_last_error().decode()
    assert L.sc_gather_batch(99, 37, 1, d_rows, None, *srcs, dev.stream, out, None, None, None, None) == -1
    # ... and a good call on the same buffers still works afterwards (the failed pointer query left no sticky error)
    rc = L.sc_gather_batch(0, 37, 1, d_rows, None, *srcs, dev.stream, out, None, None, None, None)
    assert rc == 0
    dev.sync()
    assert np.array_equal(dev.read(out, (112, 8, 8), np.float32), batch_ref.boards(src["boards"], 0))


# ------------------------------------------------------------------ against the encoder
def _encode(scamd, dev, packed, n, P, mirror, layout):
    """sc_encode_steps_device -> the device buffers (left on the device) and the status"""
    mv, off, cm, cn, coff = packed
    o = alloc_outputs(dev, P, n, layout, skip=("moves", "dist_legal" if layout else "dist"))
    rc = scamd.lib().sc_encode_steps_device(None, 0, n, _p(mv), _p(off), _p(cm), _p(cn), _p(coff), int(mirror), layout, dev.stream,
                                            o["boards"], o["meta"], o["dist"], o["dist_legal"], o["legal_idx"], o["n_legal"], o["status"])
    assert rc == 0, scamd.lib().sc_last_error().decode()
    dev.sync()
    assert not dev.read(o["status"], (n,), np.int32).any()
    return o


def test_gather_equals_the_encoders_trainer_layout(scamd, orc, dev):
    """the same games encoded as the compact source (layout 0, dist_legal) and as the trainer's tensors (layout 1, dense dist)
    without and with apply_mirror: the gather of a permutation of all rows equals expected[rows], bit for bit, for mirror = 0
    and mirror = 1 -- which ties the kernel to a path the oracle pins"""
    rnd = random.Random(4)
    games = [g for g, _ in random_games(orc, 6, 100, seed=21) if g]
    steps = [random_steps(orc, g, rnd) for g in games]
    packed = scamd.pack_steps(steps)
    n, P = len(steps), int(packed[1][-1])
    assert 150 <= P <= 600
    src = _encode(scamd, dev, packed, n, P, False, 0)
    oc = np.repeat(np.asarray([(1.0, -1.0, 0.0)[g % 3] for g in range(n)], np.float32), np.diff(packed[1].astype(np.int64)))
    src["outcome"] = dev.upload(oc)
    rows = np.random.default_rng(8).permutation(P).astype(np.int32)
    for mirror in (0, 1):
        e = _encode(scamd, dev, packed, n, P, bool(mirror), 1)
        exp = (dev.read(e["boards"], (P, 112, 8, 8), np.float32)[rows], dev.read(e["meta"], (P, 7), np.float32)[rows],
               dev.read(e["dist"], (P, 4672), np.float32)[rows], (-oc if mirror else oc)[rows])
        assert exp[2].any() and (exp[1][:, 0] == 1).any() and (exp[1][:, 0] == 0).any()
        got, n_bad = run_gather(scamd, dev, src, P, rows, np.full(P, mirror, np.uint8) if mirror else None)
        assert n_bad == 0
        assert_equal_ref(got, exp, f"mirror={mirror}")


# ------------------------------------------------------------------ the loader, with torch
_CHILD = r'''
import json, sys
import torch                      # first: libsc_engine.so then binds to the runtime torch loaded
sys.path.insert(0, sys.argv[1])
import numpy as np
import scamd
out = {}
torch.zeros(1, device="cuda:0")
sp = scamd.SelfPlay(None, n_slots=8, n_games=8, rollout_num=8, num_steps=20, evaluator="synth", temperature=1.0,
                    temperature_switch=6, seed=3, outcome_gate=4)
sp.run()
traces = [sp.trace(g) for g in range(8)]
sp.close()
steps = [[(s[0], [(c[0], c[1]) for c in s[2]]) for s in t["steps"]] for t in traces]
win = [(1.0, -1.0, 0.0)[g % 3] for g in range(8)]
S = 6
r = scamd.encode_steps_torch(steps, layout="reference", dist="both", outcomes=win)
t0 = scamd.encode_steps_torch(steps, layout="trainer", dist="dense", outcomes=win)
t1 = scamd.encode_steps_torch(steps, apply_mirror=True, layout="trainer", dist="dense", outcomes=win)
tr = [tuple(t[k] if k != "outcome" else t[k][:, None] for k in ("boards", "meta", "dist", "outcome")) for t in (t0, t1)]
lens = np.diff(r["ply_off"].astype(np.int64)).tolist()
P = sum(lens)
def eligible(games):   # global ply numbers of the reference's start_step rule, game by game
    rows = []
    for g in games:
        a, n = int(r["ply_off"][g]), lens[g]
        rows += list(range(a + (0 if n < S else S), a + n))
    return rows
same = lambda x, y: all(torch.equal(a, b) for a, b in zip(x, y))
pick = lambda t, idx: tuple(a[idx] for a in t)

rb = scamd.ReplayBuffer(P + 5, device=0, start_step=S)
rb.add(r)
el = eligible(range(8))
E = len(el)
out["E"], out["len"] = E, len(rb)
b0 = list(rb.batches(8, seed=1, epoch=0))
order, bits = rb.epoch_order(seed=1, epoch=0)
out["n_batches"] = len(b0)
out["bits_none"] = bits is None
out["rows_distinct"] = sorted(order.tolist()) == el     # nothing has wrapped: ring row = global ply
out["shapes"] = [list(x.shape) for x in b0[0]]
out["dtypes"] = [str(x.dtype) for x in b0[0]]
out["device"] = str(b0[0][0].device)
ok = True
for i, b in enumerate(b0):
    rows = order[8 * i:8 * i + 8]
    ok = ok and same(b, scamd.gather_batch_torch(rb.store, rows)) and same(b, pick(tr[0], rows.long()))
out["batches_equal_gather_and_encoder"] = bool(ok)
out["repeat_same"] = bool(all(same(x, y) for x, y in zip(b0, rb.batches(8, seed=1, epoch=0))))
o1, _ = rb.epoch_order(seed=1, epoch=1)
o2, _ = rb.epoch_order(seed=2, epoch=0)
out["next_epoch_differs"] = bool(not torch.equal(o1, order) and not torch.equal(o2, order) and sorted(o1.tolist()) == el)
# mirror: all, and one seeded bit per sample
bm = list(rb.batches(8, seed=1, epoch=0, mirror=True))
out["mirror_equal_encoder"] = bool(all(same(b, pick(tr[1], order[8 * i:8 * i + 8].long())) for i, b in enumerate(bm)))
orr, bits = rb.epoch_order(seed=1, epoch=0, mirror="random")
br = list(rb.batches(8, seed=1, epoch=0, mirror="random"))
ok = torch.equal(orr, order) and 0 < int(bits.sum()) < E
for i, b in enumerate(br):
    for j in range(8):
        k = 8 * i + j
        ok = ok and same(tuple(x[j] for x in b), tuple(a[int(orr[k])] for a in tr[int(bits[k])]))
out["random_mirror_equal_encoder"] = bool(ok)
# unshuffled with the partial batch: the eligible plies in game order
bu = list(rb.batches(8, shuffle=False, drop_last=False))
out["unshuffled"] = bool(len(bu) == -(-E // 8) and same(tuple(torch.cat(x) for x in zip(*bu)), pick(tr[0], torch.tensor(el, device="cuda:0"))))
# an add that evicts: games 0 and 1 once more; the oldest games leave, whole
it = rb.batches(8)
next(it)
r2 = scamd.encode_steps_torch(steps[:2], layout="reference", dist="legal", outcomes=win[:2])
rb.add(r2)
try:
    next(it)
    out["stale_epoch_refused"] = False
except RuntimeError:
    out["stale_epoch_refused"] = True
n_live = len(rb.index.games)
gone = 10 - n_live
out["evicted"] = gone
survivors = list(range(gone, 8)) + [0, 1]
exp = pick(tr[0], torch.tensor(eligible(survivors), device="cuda:0"))
ba = list(rb.batches(8, shuffle=False, drop_last=False))
out["after_eviction"] = bool(same(tuple(torch.cat(x) for x in zip(*ba)), exp))
live_rows = set(rb.index.eligible_rows().tolist())
bs = list(rb.batches(8, seed=5))
o5, _ = rb.epoch_order(seed=5)
out["after_eviction_shuffled"] = bool(set(o5.tolist()) == live_rows and len(bs) == len(live_rows) // 8 and
                                      all(same(b, scamd.gather_batch_torch(rb.store, o5[8 * i:8 * i + 8])) for i, b in enumerate(bs)))
# refusals by name
try:
    scamd.gather_batch_torch(t0, order[:8])
    out["trainer_refused"] = ""
except ValueError as e:
    out["trainer_refused"] = str(e)
try:
    dense = scamd.encode_steps_torch(steps[:1], layout="reference", dist="dense")
    scamd.gather_batch_torch(dense, order[:2])
    out["dense_refused"] = ""
except ValueError as e:
    out["dense_refused"] = str(e)
try:
    scamd.ReplayBuffer(lens[0] - 1).add(r)
    out["oversize"] = False
except ValueError:
    out["oversize"] = True
nb = torch.full((1,), 77, dtype=torch.int32, device="cuda:0")
bad = scamd.gather_batch_torch(r, torch.tensor([0, P, 1], device="cuda:0"), n_bad=nb)
out["n_bad"] = int(nb[0])
out["bad_row_nan"] = bool(torch.isnan(bad[2][1]).all() and torch.isnan(bad[3][1]).all() and not torch.isnan(bad[2][0]).any())
torch.cuda.synchronize()
print(json.dumps(out))
'''


def test_replay_buffer_in_a_fresh_process(scamd, tmp_path):
    """torch imported first, then scamd (a child process: this one keeps its own runtime).  About 100 eligible plies, B = 8: one
    epoch is floor(E / 8) batches over distinct rows, each equal to gather_batch_torch of its rows and to the encoder's own
    trainer-layout rows; (seed, epoch) repeats the order, another epoch or seed changes it; after an add that evicts, only rows
    of the surviving games are drawn; shapes and dtypes are the reference batch's"""
    pytest.importorskip("torch")
    out = run_torch_child(tmp_path, _CHILD, os.path.join(ROOT, "smart-chess-rust_amd"), timeout=600)
    E = out["E"]
    assert 60 <= E <= 140 and out["len"] == E, out
    assert out["n_batches"] == E // 8 and out["rows_distinct"] and out["bits_none"], out
    assert out["shapes"] == [[8, 112, 8, 8], [8, 7], [8, 4672], [8, 1]] and out["dtypes"] == ["torch.float32"] * 4, out
    assert out["device"] == "cuda:0", out
    assert out["batches_equal_gather_and_encoder"] and out["repeat_same"] and out["next_epoch_differs"], out
    assert out["mirror_equal_encoder"] and out["random_mirror_equal_encoder"] and out["unshuffled"], out
    assert out["stale_epoch_refused"] and out["evicted"] >= 1 and out["after_eviction"] and out["after_eviction_shuffled"], out
    assert "reference layout" in out["trainer_refused"] and "sparse" in out["dense_refused"] and out["oversize"], out
    assert out["n_bad"] == 1 and out["bad_row_nan"], out
