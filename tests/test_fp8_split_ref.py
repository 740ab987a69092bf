"""CPU: the yardstick of the fp8 scale tests (tests/fp8_split_ref.py), and the conditions that keep the GPU tests
(tests/test_gpu_fp8_splits.py) from passing vacuously.

The windows of lossless exponents against the brute-force rule on every tensor the GPU tests split; the blobs of every split read back
as the weights of the canonical blob; the coverage of the ramp pattern over conv index, tile and row; seven faults in the path of a
scale (a row of the wrong tile, row, conv or block, a negated or ignored exponent, a K half under another row's scale), each of which
must miss every closed form; and the CPU oracle in its fp8-emulating mode on the nets with five derived exponents a tensor."""
import numpy as np
import pytest

import fp8_split_ref as fs
import heads_ref as hr
import scw
import tail_ref as tr
import tower_ref as tw
from helpers import golden_boards

WIDTHS = (128, 256)
HEAD_NETS = ((0, 0), (1, 1), (2, 3))         # (heads_ref net, blocks) of the GPU heads test
DENSE_NETS = ((2, 128), (1, 256))


def _nets(C):
    """(label, state dict, blocks) of every net whose convs the GPU tests split"""
    yield "b", tw.net_b(C, "fp8"), 1
    yield "e2", tw.net_e2(C, "fp8")[0], 1
    yield "e1", tw.net_e1(C, "fp8")[0], 1
    yield "coarse a", fs.coarse_a(C), 1
    for off in tw.sigmas(C):
        yield f"coarse c +{off}", fs.coarse_c(C, off)[0], 1
    for k in range(3):
        yield f"coarse c, block {k + 1} of 3", fs.coarse_c(C, 0, 3, k)[0], 3
    for k, nb in HEAD_NETS:
        yield f"heads net {k}, {nb} blocks", fs.heads_net(C, k, nb), nb
    for nb, Cd in DENSE_NETS:
        if Cd == C:
            yield f"dense {nb}x{C}", fs.dense_net(nb, C), nb


def _sub(chan, pix, k):
    i = np.unique(np.linspace(0, len(chan) - 1, k).astype(int))
    return chan[i], pix[i]


def _misses(label, got, ref, bd, keep=None, alts=None):
    """the comparison of the GPU tests fails: some compared element is off by more than its bound"""
    try:
        tw.compare(label, got, ref, bd, keep, alts)
    except AssertionError:
        return True
    return False


# ---------------------------------------------------------------------------------- windows
@pytest.mark.parametrize("C", WIDTHS)
def test_windows_are_the_lossless_exponents(C):
    """every exponent inside a channel's window is lossless and the first one outside on each side is not (inside the loader's
    range), by scw.e4m3_round itself, for every e4m3 tensor of every net the GPU tests split; the two windows the probes rest on"""
    seen, widths = set(), {}
    for label, sd, nb in _nets(C):
        for name in fs.conv_names(nb):
            W = np.asarray(sd[name], np.float32)
            if W.tobytes() in seen:
                continue
            seen.add(W.tobytes())
            lo, hi = fs.window(W)
            assert (lo <= hi).all(), (label, name)
            for d in range(-1, int(np.minimum(hi - lo, 17).max()) + 2):
                e = lo + d
                inside = (e >= fs.E_MIN) & (e <= fs.E_MAX)
                ok = fs.lossless(W, np.clip(e, fs.E_MIN, fs.E_MAX))
                assert np.array_equal(ok[inside], (e <= hi)[inside] & (d >= 0)), (label, name, d)
            live = np.abs(W.reshape(len(W), -1)).max(1) > 0
            widths.setdefault(label, set()).update((hi - lo + 1)[live].tolist())
            assert np.array_equal(scw.channel_exps(W)[live], lo[live])
    print(f"C={C}: window widths of the live channels by net: " + "; ".join(f"{k}: {sorted(v)}" for k, v in widths.items()))
    grid = np.asarray([[0, 1, 2, 3, -1, -2, -3]], np.float32) / 8
    assert [int(x) for x in np.concatenate(fs.window(grid))] == [-10, 6] and [int(x) for x in np.concatenate(fs.window(np.ones((1, 1), np.float32)))] == [-8, 9]
    sd = fs.coarse_a(C)
    lo, hi = fs.window(sd["conv_block.0.weight"])
    assert set(hi - lo) == {16} and set(lo) == set(range(-12, -7)) and set(scw.channel_exps(sd["conv_block.0.weight"])) == set(range(-12, -7))


def test_quantize_refuses_a_lossy_split():
    """a given exponent outside the channel's window or the loader's range is an error; the rule's own exponents given back change nothing"""
    W = tw.net_b(128, "fp8")["conv_block.0.weight"]
    e = scw.channel_exps(W)
    for bad in (7, -11, 101, 256 - 10):          # above and below the window, outside the loader's range, -10 wrapped into a byte
        e2 = e.astype(np.int64)
        e2[5] = bad
        with pytest.raises(AssertionError):
            scw.quantize_fp8(W, e2)
    a, q, w = scw.quantize_fp8(W)
    b, q2, w2 = scw.quantize_fp8(W, e)
    assert np.array_equal(a, b) and np.array_equal(q, q2) and np.array_equal(w, w2)


@pytest.mark.parametrize("C", WIDTHS)
def test_impulse_probes_on_coarse_nets_have_bits_to_spare(C):
    """the bit comparisons of forms (a) and (c) rest on it: bias + one product fits in 21 of float32's 24 significant bits, for every
    channel, input channel and tap of the coarse convs under test (the bias grid of fp8_split_ref.coarse).  Without the grid every
    sum is still a float32 number, but channel 97 of the stem needs all 24 bits"""
    sd = fs.coarse_a(C)
    assert fs.impulse_sums_fit(sd["conv_block.0.weight"], sd["conv_block.0.bias"], 1.0, 21)
    sd = fs.coarse_a(C, bias_grid=False)
    W, b = sd["conv_block.0.weight"], sd["conv_block.0.bias"]
    assert fs.impulse_sums_fit(W, b, 1.0, 24)
    assert [c for c in range(C) if not fs.impulse_sums_fit(W[c:c + 1], b[c:c + 1], 1.0, 23)] == [97]
    for off, nb, blk in [(o, 1, 0) for o in tw.sigmas(C)] + [(0, 3, k) for k in range(3)]:
        sd, v0, v1 = fs.coarse_c(C, off, nb, blk)
        p = f"res_blocks.{blk}.conv2."
        assert fs.impulse_sums_fit(sd[p + "weight"], sd[p + "bias"], tw.r_act(v1["fp8"][0], "fp8"), 21), (off, nb, blk)


# ---------------------------------------------------------------------------------- the blobs
def test_split_blobs_read_back_as_the_canonical_weights(tmp_path):
    """read_scw(write_scw(exps=...)) gives the float32 weights of the canonical blob, for every pattern and for the extremes; the
    default export is byte for byte what it is without the argument; the splits themselves differ from the canonical one"""
    nets = [(tw.net_b(128, "fp8"), 1, 128), (fs.coarse_c(128, 16)[0], 1, 128), (fs.heads_net(256, 1, 1), 1, 256)]
    for sd, nb, C in nets:
        p0, p1 = str(tmp_path / "canon.scw"), str(tmp_path / "split.scw")
        scw.write_scw(p0, sd, nb, C, fp8=True)
        scw.write_scw(p1, sd, nb, C, fp8=True, exps={})
        assert open(p0, "rb").read() == open(p1, "rb").read()
        ref = scw.read_scw(p0)[2]
        for name in sd:
            assert np.array_equal(ref[name], np.asarray(sd[name], np.float32)), name
        for pattern in fs.PATTERNS:
            ex = fs.split(sd, nb, pattern)
            assert any((ex[n] != scw.channel_exps(sd[n])).any() for n in ex), pattern
            scw.write_scw(p1, sd, nb, C, fp8=True, exps=ex)
            assert open(p0, "rb").read() != open(p1, "rb").read()
            got = scw.read_scw(p1)
            assert got[:2] == (nb, C)
            for name in sd:
                assert np.array_equal(got[2][name].view(np.uint32), ref[name].view(np.uint32)), (pattern, name)
    sd = tw.net_a(128, "fp8")
    sx, ex = fs.extremes(sd, "conv_block.0.weight", 37, 90)
    p = str(tmp_path / "ext.scw")
    scw.write_scw(p, sx, 1, 128, fp8=True, exps=ex)
    got = scw.read_scw(p)[2]["conv_block.0.weight"]
    assert np.array_equal(got, sx["conv_block.0.weight"]) and not got[37].any() and 0 < np.abs(got[90]).max() < 2.0 ** -90


# ---------------------------------------------------------------------------------- coverage
@pytest.mark.parametrize("C", WIDTHS)
def test_ramp_reaches_every_conv_tile_and_row(C):
    """on the 3-block net of the GPU heads test: every conv index, every tile of every conv and every row-in-tile sees at least 3
    distinct exponents under `ramp`, neighbouring rows differ, adjacent convs differ at every channel, the three head convs have 8,
    8 and 4 tiles with 73 real outputs; `tiles` is constant in a tile and differs from tile to tile and from conv to conv;
    `lone` moves one channel a conv; `subnormal` leaves an e4m3 subnormal code in every channel and none below 2^-9"""
    sd = fs.heads_net(C, 2, 3)
    names = fs.conv_names(3)
    ex = fs.split(sd, 3, "ramp")
    T = fs.table(sd, ex, 3)
    assert [int((r != fs.UNWRITTEN).sum()) // 32 for r in T] == [C // 32] * 7 + [8, 8, 4] and len(ex[names[-1]]) == 73
    rows = [set() for _ in range(32)]
    for k, name in enumerate(names):
        e = ex[name].astype(int)
        assert (np.diff(e) != 0).all(), name
        for t in range(-(-len(e) // 32)):
            assert len(set(e[32 * t:32 * t + 32])) >= 3, (name, t)
        for n, v in enumerate(e):
            rows[n % 32].add(v)
        if k:
            m = min(len(e), len(ex[names[k - 1]]))
            assert (e[:m] != ex[names[k - 1]][:m]).all(), name
    assert min(len(r) for r in rows) >= 3
    print(f"C={C}: ramp exponents from {min(min(r) for r in rows)} to {max(max(r) for r in rows)}")
    ex = fs.split(sd, 3, "tiles")
    for k, name in enumerate(names):
        e = ex[name].astype(int).tolist()
        tiles = [set(e[i:i + 32]) for i in range(0, len(e), 32)]
        assert all(len(t) == 1 for t in tiles) and all(a != b for a, b in zip(tiles, tiles[1:])), name
        assert k == 0 or all(a != b for a, b in zip(tiles, [set(ex[names[k - 1]][i:i + 32].tolist()) for i in range(0, len(e), 32)])), name
    ex = fs.split(sd, 3, "lone")
    assert all((ex[n] != scw.channel_exps(sd[n])).sum() == 1 for n in names)
    ex = fs.split(sd, 3, "subnormal")
    for n in names:
        q = np.abs(np.ldexp(np.float64(sd[n]).reshape(len(ex[n]), -1), -ex[n].astype(int)[:, None]))
        assert (q[q > 0] >= 2.0 ** -9).all() and (np.where(q > 0, q, 1).min(1) <= 7 * 2.0 ** -9).all(), n


# ---------------------------------------------------------------------------------- power: every fault misses every closed form
@pytest.mark.parametrize("C", WIDTHS)
def test_wrong_scale_rules_miss_the_trunk_forms(C):
    """forms (b), (e) conv1, (e) conv2 and the coarse form (c) under `ramp`: the closed form of the weights that a faulty device
    would in effect use lies outside the bound around the closed form of the right ones, for each of the seven faults"""
    boards = tw.dense_boards(golden_boards())
    sd = tw.net_b(C, "fp8")
    ex = fs.split(sd, 1, "ramp")
    ref, bd = tw.form_b(sd, boards)
    assert not _misses("right (b)", tw.form_b(sd, boards)[0], ref, bd)
    for rule in fs.RULES:
        assert _misses(f"(b) {rule}", tw.form_b(fs.wrong(sd, ex, 1, "conv_block.0.weight", rule), boards)[0], ref, bd), rule

    sd, kap, kap1 = tw.net_e2(C, "fp8")
    ex = fs.split(sd, 1, "ramp")
    ref, bd = tw.form_e2(sd, 0, kap, kap1)
    for rule in fs.RULES:
        got = tw.form_e2(fs.wrong(sd, ex, 1, "res_blocks.0.conv2.weight", rule), 0, kap, kap1)[0]
        assert _misses(f"(e) conv2 {rule}", got[None], ref[None], bd[None]), rule

    sd, kap = tw.net_e1(C, "fp8")
    ex = fs.split(sd, 1, "ramp")
    ref, bd, keep, alts = tw.form_e1(sd, "fp8", 0, kap)
    assert not _misses("right (e) conv1", ref[None], ref[None], bd[None], keep[None], alts)
    for rule in fs.RULES:
        got = tw.form_e1(fs.wrong(sd, ex, 1, "res_blocks.0.conv1.weight", rule), "fp8", 0, kap)[0]
        assert _misses(f"(e) conv1 {rule}", got[None], ref[None], bd[None], keep[None], alts), rule

    off = tw.sigmas(C)[-1]
    sd, v0, v1 = fs.coarse_c(C, off)
    ex = fs.split(sd, 1, "ramp")
    ch, px = _sub(*tw.conv_positions(C, off), 24)
    ref, bd = tw.form_c(sd, "fp8", 0, ch, px, v0["fp8"], v1["fp8"])
    for rule in fs.RULES:
        got = tw.form_c(fs.wrong(sd, ex, 1, "res_blocks.0.conv2.weight", rule), "fp8", 0, ch, px, v0["fp8"], v1["fp8"])[0]
        assert _misses(f"coarse (c) {rule}", got, ref, bd), rule


@pytest.mark.parametrize("C", WIDTHS)
def test_wrong_scale_rules_miss_the_head_forms(orc, C):
    """form_v under a fault in the value conv, form_p under a fault in either policy conv, `ramp` on the 0-block heads net: the
    fp8-emulating oracle, fed the weights the faulty device would in effect use, misses the closed form of the right net"""
    imp = hr.impulse_positions()
    boards = np.concatenate([imp[np.unique(np.linspace(0, len(imp) - 1, 12).astype(int))], tw.dense_boards(golden_boards()), hr.random_boards(3)])
    meta = hr.metas(len(boards))
    sd = fs.heads_net(C, 1, 0)
    ex = fs.split(sd, 0, "ramp")

    def run(s):
        net = orc.Net(0, C, seed=1, emulate_fp8=True)
        for i, (name, _, _, _) in enumerate(scw.tensor_table(0, C)):
            net.set_tensor(i, np.asarray(s[name], np.float32))
        res = [net.forward(b, m) for b, m in zip(boards, meta)]
        return np.stack([r[0] for r in res]), np.asarray([r[1] for r in res], np.float32)

    ref_v, bd_v, _ = hr.form_v(sd, C, "fp8", boards, meta, k_fc2=tr.K_FC2_ORACLE)
    ref_p, bd_p = hr.form_p(sd, C, "fp8", boards)
    lp, v = run(sd)
    assert not _misses("right (v)", v, ref_v, bd_v) and not _misses("right (p)", lp, ref_p, bd_p)
    for rule in fs.RULES:
        assert _misses(f"(v) {rule}", run(fs.wrong(sd, ex, 0, "value_head.conv.0.weight", rule))[1], ref_v, bd_v), rule
        for name in ("policy_head.model.0.weight", "policy_head.model.2.weight"):
            assert _misses(f"(p) {name} {rule}", run(fs.wrong(sd, ex, 0, name, rule))[0], ref_p, bd_p), (name, rule)


# ---------------------------------------------------------------------------------- the oracle on five exponents a tensor
@pytest.mark.parametrize("C", WIDTHS)
def test_oracle_meets_the_forms_on_derived_exponents(orc, C):
    """the shifted form (a) and the coarse form (c), in block 1 of 1 and in block 2 of 3: the oracle's fp8-emulating mode, which derives
    the five exponents of a tensor by its own rule, lies inside the same bounds"""
    sd = fs.coarse_a(C)
    tw.representable(sd, "fp8")
    pl, px = _sub(*tw.stem_positions(), 40)
    ref, bd = tw.form_a(sd, "fp8", pl, px)
    tw.compare(f"oracle {C} fp8 shifted (a)", fs.oracle_latents(orc, sd, 0, C, tw.impulse_board(pl, px)), ref, bd)
    off = tw.sigmas(C)[-1]
    ch, px = _sub(*tw.conv_positions(C, off), 24)
    for nb, blk in ((1, 0), (3, 1)):
        sd, v0, v1 = fs.coarse_c(C, off, nb, blk)
        tw.representable(sd, "fp8")
        ref, bd = tw.form_c(sd, "fp8", blk, ch, px, v0["fp8"], v1["fp8"])
        tw.compare(f"oracle {C} fp8 coarse (c), block {blk + 1} of {nb}", fs.oracle_latents(orc, sd, nb, C, tw.impulse_board(ch - off, px)), ref, bd)
    sd = tw.net_a(C, "fp8")
    sx, _ = fs.extremes(sd, "conv_block.0.weight", tw.chan8(C)[3], tw.chan8(C)[5])
    pl, px = _sub(*tw.stem_positions(), 12)
    ref, bd = tw.form_a(sx, "fp8", pl, px)
    tw.compare(f"oracle {C} fp8 (a), a dead and a tiny channel", fs.oracle_latents(orc, sx, 0, C, tw.impulse_board(pl, px)), ref, bd)
