"""Identical training positions merged on the GPU (-m gpu): sc_merge_positions against the numpy yardstick (tests/merge_ref.py),
bit for bit -- there is no tolerance in this feature.  Device buffers come from hipMalloc on the HIP runtime libsc_engine.so uses
(ctypes), pre-filled with 0x5a, and the stream is not the default one: this file does not import torch; the replay buffer on top
runs in a child process that imports torch before scamd."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import batch_ref
import merge_ref
from helpers import random_games, random_steps
from support import FILL, ROOT, _p, open_dev, run_torch_child, scamd_gpu, untouched  # noqa: F401

pytestmark = pytest.mark.gpu
KEYS = merge_ref.KEYS
OUT = KEYS + ("count", "first")
ROW_BYTES = dict(boards=7168, meta=28, dist_legal=896, legal_idx=448, n_legal=4, outcome=4, count=4, first=4)
SHAPES = dict(boards=((8, 8, 112), np.int8), meta=((7,), np.int32), dist_legal=((224,), np.float32), legal_idx=((224,), np.uint16),
              n_legal=((), np.int32), outcome=((), np.float32), count=((), np.int32), first=((), np.int32))
FILL32 = int.from_bytes(bytes([FILL] * 4), "little")


@pytest.fixture(scope="module")
def dev(scamd):
    yield from open_dev(scamd, FILL)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def upload(dev, src):
    return {k: dev.upload(src[k]) for k in KEYS}


def run_merge(scamd, dev, d_src, n_src, n_in, rows=None, key_bits=128, skip=(), expect_rc=0, ws_short=0, extra_rows=0):
    """sc_merge_positions on the non-default stream into 0x5a-filled buffers of n_in + extra_rows rows -> what the buffers hold
    afterwards (whole, unsliced), group_of and counts"""
    L = scamd.lib()
    need = C.c_size_t(0)
    assert L.sc_merge_positions_workspace(n_in, C.byref(need)) == 0
    ws = dev.alloc(need.value)
    cap = n_in + extra_rows
    outs = {k: (None if k in skip else dev.alloc(cap * ROW_BYTES[k])) for k in OUT}
    group_of = None if "group_of" in skip else dev.alloc(n_in * 4)
    counts = None if "counts" in skip else dev.alloc(16)
    d_rows = None if rows is None else dev.upload(np.asarray(rows, np.int32))
    rc = L.sc_merge_positions(0, n_src, n_in, d_rows, *[d_src[k] for k in KEYS], key_bits, ws, need.value - ws_short, dev.stream,
                              *[outs[k] for k in OUT], group_of, counts)
    assert rc == expect_rc, L.sc_last_error().decode()
    dev.sync()
    got = {k: dev.read(outs[k], (cap,) + SHAPES[k][0], SHAPES[k][1]) for k in OUT if outs[k] is not None}
    g = None if group_of is None else dev.read(group_of, (n_in,), np.int32)
    c = None if counts is None else dev.read(counts, (4,), np.int32)
    return got, g, c


def assert_equals_ref(got, g, c, ref, what=""):
    exp, exp_g, exp_c = ref
    G = int(exp_c[0])
    assert c.tolist() == exp_c.tolist(), (what, c, exp_c)
    assert _same(g, exp_g), what
    for k in OUT:
        assert _same(got[k][:G], exp[k]), (what, k)
        assert untouched(got[k][G:]), (what, k, "rows past the groups")


# ------------------------------------------------------------------ 1: all distinct
def test_distinct_rows_come_back_bit_for_bit(scamd, dev):
    src = merge_ref.make_source()
    got, g, c = run_merge(scamd, dev, upload(dev, src), 37, 37, extra_rows=3)
    assert c.tolist() == [37, 0, 0, 1]
    assert g.tolist() == list(range(37))
    for k in KEYS:
        assert _same(got[k][:37], src[k]), k
        assert untouched(got[k][37:]), k
    assert (got["count"][:37] == 1).all() and got["first"][:37].tolist() == list(range(37))
    assert_equals_ref(got, g, c, merge_ref.merge(src))


# ------------------------------------------------------------------ 2: duplicates
def _copies():
    copies = [1 + (r * 7) % 11 for r in range(37)]
    copies[3], copies[10] = 65, 130   # n_legal 64 and 0: out_count and counts[3] cross 64 and 128
    return copies


@pytest.fixture(scope="module")
def duplicates(dev):
    src, origin = merge_ref.expand(merge_ref.make_source(), _copies())
    assert 380 <= len(origin) <= 520
    assert {int(src["n_legal"][p]) for p in range(len(origin))} == set(merge_ref.N_LEGAL)
    return src, upload(dev, src), merge_ref.merge(src)


def test_duplicates_are_merged_as_the_yardstick_merges_them(scamd, dev, duplicates):
    src, d_src, ref = duplicates
    n = src["boards"].shape[0]
    assert ref[2].tolist() == [37, 0, 0, 130] and sorted(ref[0]["count"].tolist())[-2:] == [65, 130]
    first = run_merge(scamd, dev, d_src, n, n)
    assert_equals_ref(*first, ref)
    again = run_merge(scamd, dev, d_src, n, n)
    for k in OUT:
        assert _same(first[0][k], again[0][k]), k
    assert _same(first[1], again[1]) and _same(first[2], again[2])


# ------------------------------------------------------------------ 3: every byte counts
def test_every_byte_of_the_sample_counts(scamd, dev):
    rng = np.random.default_rng(5)
    base = merge_ref.make_source(10, seed=9)
    r = 9
    assert base["n_legal"][r] == 218
    n_var = 7168 + 28 + 218 + 1 + 16
    where = (0, n_var // 2, n_var + 2)   # the base at the first, a middle and the last position
    n = n_var + 3
    src = {k: np.repeat(base[k][r:r + 1], n, axis=0) for k in KEYS}
    var = [p for p in range(n) if p not in where]
    bb = src["boards"].reshape(n, 7168).view(np.uint8)
    mb = src["meta"].view(np.uint8).reshape(n, 28)
    v = 0
    for i in range(7168):
        bb[var[v], i] ^= 1 << (i % 8)
        v += 1
    for i in range(28):
        mb[var[v], i] ^= 1 << (i % 8)
        v += 1
    for i in range(218):
        src["legal_idx"][var[v], i] ^= 1 << (i % 16)
        v += 1
    src["n_legal"][var[v]] = 217
    v += 1
    unequal = np.flatnonzero(bb[where[0], :-1] != bb[where[0], 1:])
    for i in rng.choice(unequal, 16, replace=False):   # two unequal neighbouring bytes exchanged
        p = var[v]
        bb[p, i], bb[p, i + 1] = bb[p, i + 1], bb[p, i]
        v += 1
    assert v == n_var
    merge_ref.fresh_targets(src, rng, rows=where)
    ref_g, groups, _ = merge_ref.partition(src)
    assert len(groups) == n_var + 1 and groups[0] == list(where) and all(len(x) == 1 for x in groups[1:])
    got, g, c = run_merge(scamd, dev, upload(dev, src), n, n, skip=("boards", "meta", "legal_idx", "n_legal", "count", "first"))
    assert c.tolist() == [n_var + 1, 0, 0, 3]
    assert _same(g, ref_g)
    exp = merge_ref.merged_rows(src, groups[:1])
    assert _same(got["dist_legal"][:1], exp["dist_legal"]) and _same(got["outcome"][:1], exp["outcome"])
    rest = [x[0] for x in groups[1:]]
    assert _same(got["dist_legal"][1:n_var + 1], src["dist_legal"][rest]) and _same(got["outcome"][1:n_var + 1], src["outcome"][rest])


# ------------------------------------------------------------------ 4: keys are only a shortcut
@pytest.mark.parametrize("key_bits", [0, 1, 4, 128])
def test_the_byte_compare_decides_whatever_the_key(scamd, dev, duplicates, key_bits):
    src, d_src, ref = duplicates
    n = src["boards"].shape[0]
    got, g, c = run_merge(scamd, dev, d_src, n, n, key_bits=key_bits)
    G = int(c[0])
    assert (g >= 0).all() and sorted(set(g.tolist())) == list(range(G))            # a partition of the positions
    groups = [np.flatnonzero(g == j).tolist() for j in range(G)]
    heads = [x[0] for x in groups]
    assert heads == sorted(heads) and got["first"][:G].tolist() == heads            # numbered by ascending head
    for members in groups:                                                          # members of a group are byte-equal
        assert len({merge_ref.sample_bytes(src, p) for p in members}) == 1
    exp = merge_ref.merged_rows(src, groups)   # the yardstick's arithmetic on the device's own partition
    for k in OUT:
        assert _same(got[k][:G], exp[k]), k
        assert untouched(got[k][G:]), k
    assert c[1] == 0 and c[3] == max(len(x) for x in groups)
    # a group is a whole class of the yardstick or a single position; a position split off its class is a counted key clash
    split = 0
    for members in groups:
        cls = np.flatnonzero(ref[1] == ref[1][members[0]]).tolist()
        assert members == cls or len(members) == 1
        split += members != cls
    assert split <= c[2] <= n - max(len(x) for x in groups)
    if key_bits == 0:     # one key: the class of position 0 is merged, every other position is alone
        cls = np.flatnonzero(ref[1] == ref[1][0]).tolist()
        assert groups[0] == cls and all(len(x) == 1 for x in groups[1:]) and c[2] == n - len(cls)
    if key_bits == 128:
        assert c[2] == 0 and _same(g, ref[1])


# ------------------------------------------------------------------ 5: rows
def test_rows_select_repeat_and_contain_bad_input(scamd, dev):
    src = merge_ref.make_source(40, seed=3)
    src["n_legal"][7], src["n_legal"][8] = -1, 219
    n_src = 40
    rng = np.random.default_rng(6)
    rows = rng.permutation(n_src)[:25].tolist()
    rows = [r for r in rows if r not in (7, 8, 11)] + [7, 8, 11, 11, -1, n_src, 2 ** 31 - 1, -2 ** 31]
    rng.shuffle(rows)
    ref = merge_ref.merge(src, rows)
    got, g, c = run_merge(scamd, dev, upload(dev, src), n_src, len(rows), rows=rows)
    assert_equals_ref(got, g, c, ref, "rows")
    assert c[1] == 6 and c[3] == 2 and c[2] == 0
    assert (g[[i for i, r in enumerate(rows) if not 0 <= r < n_src]] == -1).all() and (g >= -1).all()
    j = int(g[rows.index(11)])
    assert got["count"][j] == 2
    for k in KEYS:   # the mean of a row with itself is the row: (x + x) / 2, exactly
        assert _same(got[k][j], src[k][11]), k
    for r in (7, 8):   # verbatim groups of one
        j = int(g[rows.index(r)])
        assert got["count"][j] == 1 and all(_same(got[k][j], src[k][r]) for k in KEYS)


# ------------------------------------------------------------------ 6: edges
def test_edges(scamd, dev):
    src = merge_ref.make_source(4, seed=4)
    d_src = upload(dev, src)
    got, g, c = run_merge(scamd, dev, d_src, 4, 0, extra_rows=2)
    assert c.tolist() == [0, 0, 0, 0] and all(untouched(got[k]) for k in OUT)
    got, g, c = run_merge(scamd, dev, d_src, 4, 1)
    assert_equals_ref(got, g, c, merge_ref.merge(src, n_in=1), "one")
    assert c.tolist() == [1, 0, 0, 1]
    got, g, c = run_merge(scamd, dev, d_src, 4, 2)
    assert_equals_ref(got, g, c, merge_ref.merge(src, n_in=2), "two unequal")
    assert c.tolist() == [2, 0, 0, 1]
    twin = {k: src[k][[1, 1]].copy() for k in KEYS}
    merge_ref.fresh_targets(twin, np.random.default_rng(1))
    got, g, c = run_merge(scamd, dev, upload(dev, twin), 2, 2)
    assert_equals_ref(got, g, c, merge_ref.merge(twin), "two equal")
    assert c.tolist() == [1, 0, 0, 2]


# ------------------------------------------------------------------ 7: refusals
def test_null_outputs_and_refusals(scamd, dev, duplicates):
    src, d_src, ref = duplicates
    n = src["boards"].shape[0]
    for skip in OUT + ("group_of", "counts"):
        got, g, c = run_merge(scamd, dev, d_src, n, n, skip=(skip,))
        for k in OUT:
            if k != skip:
                assert _same(got[k][:37], ref[0][k]), (skip, k)
        assert skip == "group_of" or _same(g, ref[1]), skip
        assert skip == "counts" or c.tolist() == ref[2].tolist(), skip
    L = scamd.lib()
    need = C.c_size_t(0)
    assert L.sc_merge_positions_workspace(n, C.byref(need)) == 0
    ws = dev.alloc(need.value)
    counts = dev.alloc(16)
    srcs = [d_src[k] for k in KEYS]
    nulls = [None] * 9
    host_ws, host_counts = np.zeros(need.value, np.uint8), np.zeros(4, np.int32)
    assert L.sc_merge_positions(0, n, n, None, *srcs, 128, _p(host_ws), need.value, dev.stream, *nulls, counts) == -1
    assert "workspace" in L.sc_last_error().decode() and "device memory" in L.sc_last_error().decode()
    assert L.sc_merge_positions(0, n, n, None, *srcs, 128, ws, need.value, dev.stream, *nulls, _p(host_counts)) == -1
    assert "counts" in L.sc_last_error().decode()
    assert L.sc_merge_positions(0, n, n, None, _p(src["boards"]), *srcs[1:], 128, ws, need.value, dev.stream, *nulls, counts) == -1
    assert "boards" in L.sc_last_error().decode()
    assert L.sc_merge_positions(0, n, n, None, *srcs, 128, ws, need.value - 1, dev.stream, *nulls, counts) == -1
    assert "workspace" in L.sc_last_error().decode()
    assert L.sc_merge_positions(99, n, n, None, *srcs, 128, ws, need.value, dev.stream, *nulls, counts) == -1
    dev.sync()
    assert untouched(dev.read(counts, (4,), np.int32))   # nothing was enqueued by a refused call
    assert L.sc_merge_positions(0, n, n, None, *srcs, 128, ws, need.value, dev.stream, *nulls, counts) == 0
    dev.sync()
    assert dev.read(counts, (4,), np.int32).tolist() == ref[2].tolist()


# ------------------------------------------------------------------ 8: encoder data
def test_encoded_games_with_twins(scamd, orc, dev):
    """every game encoded twice in one call, with visit counts of its own each time: every ply has a twin, ply 0 is one large
    group; the merged rows feed sc_gather_batch"""
    rnd = random.Random(7)
    games = [g for g, _ in random_games(orc, 5, 50, seed=23) if g]
    steps = [random_steps(orc, g, rnd) for g in games]
    steps += [[(m, [(c, rnd.randint(0, 200)) for c, _ in ch]) for m, ch in st] for st in steps]
    mv, off, cm, cn, coff = scamd.pack_steps(steps)
    n, P = len(steps), int(off[-1])
    assert 60 <= P <= 500
    o = {k: dev.alloc(P * ROW_BYTES[k]) for k in KEYS if k != "outcome"}
    status = dev.alloc(n * 4)
    rc = scamd.lib().sc_encode_steps_device(None, 0, n, _p(mv), _p(off), _p(cm), _p(cn), _p(coff), 0, 0, dev.stream, o["boards"], o["meta"],
                                            None, o["dist_legal"], o["legal_idx"], o["n_legal"], status)
    assert rc == 0, scamd.lib().sc_last_error().decode()
    dev.sync()
    assert not dev.read(status, (n,), np.int32).any()
    src = {k: dev.read(o[k], (P,) + SHAPES[k][0], SHAPES[k][1]) for k in o}
    src["outcome"] = np.repeat(np.asarray([(1.0, -1.0, 0.0)[g % 3] for g in range(n)], np.float32), np.diff(off.astype(np.int64)))
    o["outcome"] = dev.upload(src["outcome"])
    ref = merge_ref.merge(src)
    G = int(ref[2][0])
    assert (ref[0]["count"] >= 2).all() and ref[0]["count"][0] == n and G <= P // 2
    got, g, c = run_merge(scamd, dev, o, P, P)
    assert_equals_ref(got, g, c, ref, "encoder")
    # the merged rows as a source of minibatches
    d_m = {k: dev.upload(got[k][:G]) for k in KEYS}
    rows = np.random.default_rng(3).permutation(G).astype(np.int32)
    outs = [dev.alloc(G * s) for s in (7168 * 4, 28, 4672 * 4, 4)]
    n_bad = dev.alloc(4)
    rc = scamd.lib().sc_gather_batch(0, G, G, dev.upload(rows), None, *[d_m[k] for k in KEYS], dev.stream, *outs, n_bad)
    assert rc == 0, scamd.lib().sc_last_error().decode()
    dev.sync()
    exp = batch_ref.gather(ref[0], rows)
    assert exp[4] == 0 and dev.read(n_bad, (1,), np.int32)[0] == 0
    for buf, shape, e in zip(outs, ((G, 112, 8, 8), (G, 7), (G, 4672), (G,)), exp):
        assert _same(dev.read(buf, shape, np.float32), e)


# ------------------------------------------------------------------ a size at which the sort takes its other path
def test_two_million_positions_over_few_rows(scamd, dev):
    """2^21 + 3 positions that stand for 37 source rows (rows repeat): the table, the scan and the member walk at a size where
    the radix sort no longer runs as a merge sort.  The large outputs hold only the 37 rows the call may write.  The yardstick
    here is vectorised: a group is the positions of one source row, and np.cumsum is numpy's sequential float32 sum"""
    src = merge_ref.make_source()
    n = (1 << 21) + 3
    rows = np.random.default_rng(11).integers(0, 37, n).astype(np.int32)
    first = np.full(37, n, np.int64)
    np.minimum.at(first, rows, np.arange(n))
    order = np.argsort(first)                      # source rows by their first position
    rank = np.empty(37, np.int32)
    rank[order] = np.arange(37, dtype=np.int32)
    L = scamd.lib()
    need = C.c_size_t(0)
    assert L.sc_merge_positions_workspace(n, C.byref(need)) == 0
    ws = dev.alloc(need.value)
    outs = {k: dev.alloc(37 * ROW_BYTES[k]) for k in OUT}
    group_of, counts = dev.alloc(n * 4), dev.alloc(16)
    d_src = upload(dev, src)
    rc = L.sc_merge_positions(0, 37, n, dev.upload(rows), *[d_src[k] for k in KEYS], 128, ws, need.value, dev.stream,
                              *[outs[k] for k in OUT], group_of, counts)
    assert rc == 0, L.sc_last_error().decode()
    dev.sync()
    m = np.bincount(rows, minlength=37)[order]
    assert dev.read(counts, (4,), np.int32).tolist() == [37, 0, 0, int(m.max())]
    assert _same(dev.read(group_of, (n,), np.int32), rank[rows])
    got = {k: dev.read(outs[k], (37,) + SHAPES[k][0], SHAPES[k][1]) for k in OUT}
    assert got["count"].tolist() == m.tolist() and got["first"].tolist() == first[order].tolist()
    for k in ("boards", "meta", "legal_idx", "n_legal"):
        assert _same(got[k], src[k][order]), k
    for j, r in enumerate(order):
        nl = int(src["n_legal"][r])
        x = np.append(src["dist_legal"][r, :nl], src["outcome"][r]).astype(np.float32)
        s = np.cumsum(np.broadcast_to(x, (int(m[j]), nl + 1)), axis=0, dtype=np.float32)[-1]
        mean = (s / np.float32(m[j])).astype(np.float32)
        assert _same(got["dist_legal"][j, :nl], mean[:nl]) and _same(got["dist_legal"][j, nl:], src["dist_legal"][r, nl:]), j
        assert _same(got["outcome"][j:j + 1], mean[nl:]), j


# ------------------------------------------------------------------ group heads at the edges of the scan's tiles
def test_group_heads_at_the_scan_tile_edges(scamd, dev):
    """257 * 1024 + 2 positions -- more tiles than the scan's sums kernel carries in one round, the last tile of two -- over 13
    source rows that first appear at the first, second and last position of tiles 0, 1, 256 and 257: every tile carry and every
    in-tile offset the group numbers depend on is non-zero somewhere.  Only the small outputs are asked for; the yardstick is
    numpy, over every position"""
    T = 1024
    n = 257 * T + 2
    heads = np.array([0, 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 256 * T - 1, 256 * T, 256 * T + 1, 257 * T - 1, 257 * T, n - 1], np.int64)
    src = merge_ref.make_source(13)
    seen = np.searchsorted(heads, np.arange(n), side="left")           # the source rows that appeared before position p
    rows = (np.random.default_rng(17).random(n) * seen).astype(np.int32)   # one of them (position 0 is a head)
    rows[heads] = np.arange(13, dtype=np.int32)
    first = np.full(13, n, np.int64)
    np.minimum.at(first, rows, np.arange(n))
    assert first.tolist() == heads.tolist()                             # row j is new at heads[j] and nowhere earlier
    L = scamd.lib()
    need = C.c_size_t(0)
    assert L.sc_merge_positions_workspace(n, C.byref(need)) == 0
    ws = dev.alloc(need.value)
    outs = {k: (dev.alloc(13 * ROW_BYTES[k]) if k in ("count", "first") else None) for k in OUT}
    group_of, counts = dev.alloc(n * 4), dev.alloc(16)
    d_src = upload(dev, src)
    rc = L.sc_merge_positions(0, 13, n, dev.upload(rows), *[d_src[k] for k in KEYS], 128, ws, need.value, dev.stream,
                              *[outs[k] for k in OUT], group_of, counts)
    assert rc == 0, L.sc_last_error().decode()
    dev.sync()
    m = np.bincount(rows, minlength=13)
    assert dev.read(counts, (4,), np.int32).tolist() == [13, 0, 0, int(m.max())]
    assert _same(dev.read(group_of, (n,), np.int32), rows)              # rank by first appearance = the row's own number here
    assert dev.read(outs["first"], (13,), np.int32).tolist() == heads.tolist()
    assert dev.read(outs["count"], (13,), np.int32).tolist() == m.tolist()


# ------------------------------------------------------------------ 9: the loader, with torch
_CHILD = r'''
import json, sys
import torch                      # first: libsc_engine.so then binds to the runtime torch loaded
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import numpy as np
import scamd
from scamd import replay
import merge_ref
out = {}
torch.zeros(1, device="cuda:0")
sp = scamd.SelfPlay(None, n_slots=8, n_games=8, rollout_num=8, num_steps=20, evaluator="synth", temperature=1.0,
                    temperature_switch=6, seed=3, outcome_gate=4)
sp.run()
traces = [sp.trace(g) for g in range(8)]
sp.close()
steps = [[(s[0], [(c[0], c[1]) for c in s[2]]) for s in t["steps"]] for t in traces]
steps = steps + steps[:4]          # four games twice: every ply of theirs has a twin
win = [(1.0, -1.0, 0.0)[g % 3] for g in range(len(steps))]
r = scamd.encode_steps_torch(steps, layout="reference", dist="both", outcomes=win)
KEYS = merge_ref.KEYS
host = {k: r[k].cpu().numpy() for k in KEYS}
host["legal_idx"] = host["legal_idx"].view(np.uint16)
P = host["boards"].shape[0]
same = lambda x, y: all(torch.equal(a, b) for a, b in zip(x, y))
bits = lambda t: t.contiguous().cpu().numpy().tobytes()

# the function itself against the yardstick
m = replay.merge_positions_torch(r)
ref, ref_g, ref_c = merge_ref.merge(host)
G = int(ref_c[0])
out["G"], out["P"] = G, P
out["merge_equals_yardstick"] = bool(all(bits(m[k]) == ref[k].tobytes() for k in KEYS) and bits(m["count"]) == ref["count"].tobytes()
                                     and bits(m["first"]) == ref["first"].tobytes() and bits(m["group_of"]) == ref_g.tobytes()
                                     and m["n_bad"] == 0 and m["n_key_clash"] == 0 and m["boards"].shape[0] == G)
u = replay.unique_by_ply(m)
lens = np.diff(np.asarray(r["ply_off"], np.int64))
L = int(lens.max())
plies = [int((lens > k).sum()) for k in range(L)]
off = np.asarray(r["ply_off"], np.int64)
distinct = [len({int(ref_g[off[g] + k]) for g in range(len(lens)) if lens[g] > k}) for k in range(L)]
out["unique_by_ply"] = bool(u["plies"].tolist() == plies and u["distinct"].tolist() == distinct)
out["ply0"] = [int(u["plies"][0]), int(u["distinct"][0])]

# the buffer: before-the-change behaviour of unique=False is the order of epoch_order and gather_batch_torch of its rows
S = 2
rb = scamd.ReplayBuffer(P + 5, device=0, start_step=S)
rb.add(r)
order, _ = rb.epoch_order(seed=1, epoch=0)
gen = torch.Generator(device="cuda:0")
gen.manual_seed(scamd.ReplayIndex.epoch_seed(1, 0))
el = torch.from_numpy(rb.index.eligible_rows()).to("cuda:0")
old_order = el[torch.randperm(el.shape[0], generator=gen, device="cuda:0")].to(torch.int32)
b0 = list(rb.batches(8, seed=1, epoch=0))
out["plain_unchanged"] = bool(torch.equal(order, old_order) and len(b0) == el.shape[0] // 8 and
                              all(same(b, scamd.gather_batch_torch(rb.store, old_order[8 * i:8 * i + 8])) for i, b in enumerate(b0)))
mg = rb.merged()
rows = rb.index.eligible_rows()
ref, ref_g, ref_c = merge_ref.merge(host, rows)      # nothing has wrapped: ring row = global ply
G = int(ref_c[0])
out["merged_equals_yardstick"] = bool(all(bits(mg[k]) == ref[k].tobytes() for k in KEYS) and bits(mg["group_of"]) == ref_g.tobytes())
out["merged_is_kept"] = rb.merged() is mg
uo, _ = rb.epoch_order(seed=1, epoch=0, unique=True)
bu = list(rb.batches(8, seed=1, epoch=0, unique=True, drop_last=False))
out["covers_every_group_once"] = bool(sorted(uo.tolist()) == list(range(G)) and sum(b[0].shape[0] for b in bu) == G)
out["unique_equals_gather"] = bool(all(same(b, scamd.gather_batch_torch(mg, uo[8 * i:8 * i + 8])) for i, b in enumerate(bu)))
out["E"], out["G_buffer"] = int(len(rows)), G
ub = replay.unique_by_ply(mg)
first = [0 if n < S else S for n in lens]
Lb = max(int(n) for n in lens)
pl = [sum(1 for g in range(len(lens)) if first[g] <= k < lens[g]) for k in range(Lb)]
pos_of = {}
i = 0
for g in range(len(lens)):
    for k in range(first[g], int(lens[g])):
        pos_of[(g, k)] = i
        i += 1
di = [len({int(ref_g[pos_of[(g, k)]]) for g in range(len(lens)) if (g, k) in pos_of}) for k in range(Lb)]
out["buffer_unique_by_ply"] = bool(ub["plies"].tolist() == pl and ub["distinct"].tolist() == di)
# an add invalidates the merge like the epoch
it = rb.batches(8, unique=True)
next(it)
rb.add(scamd.encode_steps_torch(steps[:1], layout="reference", dist="legal", outcomes=win[:1]))
try:
    next(it)
    out["stale_epoch_refused"] = False
except RuntimeError:
    out["stale_epoch_refused"] = True
out["merge_redone_after_add"] = bool(rb.merged() is not mg and int(rb.merged()["count"].sum()) == len(rb))
torch.cuda.synchronize()
print(json.dumps(out))
'''


def test_replay_buffer_unique_in_a_fresh_process(scamd, tmp_path):
    """torch imported first, then scamd (a child process: this one keeps its own runtime)"""
    pytest.importorskip("torch")
    out = run_torch_child(tmp_path, _CHILD, os.path.join(ROOT, "smart-chess-rust_amd"), os.path.join(ROOT, "tests"), timeout=600)
    assert out["G"] < out["P"] and out["G_buffer"] < out["E"], out
    assert out["merge_equals_yardstick"] and out["unique_by_ply"] and out["ply0"] == [12, 1], out
    assert out["plain_unchanged"] and out["merged_equals_yardstick"] and out["merged_is_kept"], out
    assert out["covers_every_group_once"] and out["unique_equals_gather"] and out["buffer_unique_by_ply"], out
    assert out["stale_epoch_refused"] and out["merge_redone_after_add"], out
