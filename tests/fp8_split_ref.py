"""The yardstick of the fp8 scale tests: many exponent splits of the same real weights.

The fp8 tower carries one power-of-two scale per output channel.  An SCW2 blob stores it as an exponent byte per channel
(tools/scw.py), `pack8` (csrc/weights.hpp) turns it into a row of the E8M0 scale table [conv][8 tiles][64 lanes], `scale_load`
(csrc/nn_tower32.hpp) fetches that row one conv ahead of its use and the matrix instruction takes it as the scale of its A rows.
Seeded weights give every channel of a tensor the same exponent, so a row read from the wrong conv, tile, lane or block does not show
on them.  Here the exponents are chosen by hand.

THE IDEA.  A weight w can be written as q 2^e with q in e4m3 for several e: the 1/8 grid {0, +-1, +-2, +-3} / 8 of the exact-sum
probes for every e in [-10, 6] (at the upper end q is an e4m3 subnormal), the weight 1 of the pass-through and identity convs for
every e in [-8, 9].  `window` gives the interval per output channel.  All splits of a tensor stand for the same real weights, so
whatever split each channel uses, the device must meet the float64 closed forms of tests/tower_ref.py and tests/heads_ref.py within
their bounds, and on the probes whose partial sums are all exact (impulse and exact-sum probes) it must return the bits of the
canonical split.  No tolerance is new: every bound is the one tower_ref / heads_ref computes.

  * `coarse` makes a natural conv splittable: channel c becomes rint(3 W[c] / max|W[c]|) / 8 2^s_c with s_c from -2..2 (the bias
    scaled alike), so the exponents that the loader derives span five values in a tensor and every channel has a 17-wide window.
  * `split` chooses the exponents of every conv of a net by a pattern over (conv index k, channel n): PATTERNS.
  * `extremes` puts a dead channel (all-zero codes) at exponent +100 and a live one at -100, the ends of the loader's range.
  * `wrong` gives the weights that a device with one of seven faults in the path of the scale (RULES) would in effect use;
    tests/test_fp8_split_ref.py shows that each of them misses every closed form under the patterns used.

Plain numpy; nothing of the engine or the oracle is imported (`oracle_latents` and `engine_from_split` take them as arguments)."""
import numpy as np

import heads_ref as hr
import scw
import tower_ref as tw

E_MIN, E_MAX = -100, 100           # the loader's range of a channel exponent (csrc/weights.hpp: load_scw)
UNWRITTEN = -127                   # a byte 0 of the scale table: a tile that no conv of that index has
PATTERNS = ("ramp", "tiles", "lone", "subnormal")
RULES = ("tile^1", "row+1", "next conv", "previous block", "negated", "ignored", "upper K half")
SEED = 71


def conv_names(nb):
    """the e4m3 conv tensors in the order of the scale table: conv index 0 the stem, 1 + 2b / 2 + 2b block b, then the three head convs"""
    n = ["conv_block.0.weight"]
    for b in range(nb):
        n += [f"res_blocks.{b}.conv1.weight", f"res_blocks.{b}.conv2.weight"]
    return n + ["value_head.conv.0.weight", "policy_head.model.0.weight", "policy_head.model.2.weight"]


# ------------------------------------------------------------------ windows
def window(w):
    """per output channel the interval [lo, hi] of exponents e for which w / 2^e is e4m3 without loss, clipped to the loader's range
    (an all-zero channel: the whole range; lo > hi: no such exponent).  A value odd 2^k of at most 4 significant bits is e4m3 at e
    iff k - e >= -9 (the subnormal quantum) and |w| / 2^e <= 448: hi = min k + 9, lo the exponent of scw.channel_exps"""
    w = np.asarray(w, np.float32)
    a = np.abs(w.reshape(w.shape[0], -1)).astype(np.float64)
    f, ex = np.frexp(a)
    m = np.rint(np.ldexp(f, 24)).astype(np.int64)                  # float32: 24 significant bits
    live = m > 0
    tz = np.where(live, np.rint(np.log2(np.maximum(m & -m, 1))).astype(np.int64), 24)
    k = np.where(live, ex - 24 + tz, 10 ** 6)
    lo = scw.channel_exps(w).astype(np.int64)
    hi = np.minimum(k.min(1) + 9, E_MAX)
    hi = np.where(np.where(live, 24 - tz, 0).max(1) > 4, lo - 1, hi)
    dead = ~live.any(1)
    return np.where(dead, E_MIN, lo), np.where(dead, E_MAX, hi)


def lossless(w, e):
    """bool[O]: w[c] / 2^e[c] is e4m3 without loss -- the brute-force rule the windows are checked against"""
    w = np.asarray(w, np.float32)
    with np.errstate(over="ignore"):
        x = np.ldexp(w.reshape(w.shape[0], -1), -np.asarray(e, np.int32)[:, None])
    return (scw.e4m3_round(x) == x).all(1)


# ------------------------------------------------------------------ splittable natural convs
def draw_shifts(sd, names, seed):
    """name -> s[O]: the five values -2..2 in equal shares, shuffled"""
    r = np.random.default_rng(seed)
    return {n: r.permutation(np.arange(np.shape(sd[n])[0]) % 5 - 2) for n in names}


BIAS_GRID = 2.0 ** -16


def coarse(sd, names, shifts, bias_grid=True):
    """in place: W[c] <- rint(3 W[c] / max|W[c]|) / 8 2^s_c for every conv weight in names, its bias scaled by the same 2^s_c; the
    canonical exponent of channel c becomes s_c - 10 and its window [s_c - 10, s_c + 6].  bias_grid: the bias is first put on the
    2^-16 grid (a seeded bf16 bias of 2^-9 or more lies on it already), so that bias + one product fits in 21 of float32's 24
    significant bits (`impulse_sums_fit`).  Without it a bias of 2^-19 beside a weight of 2^-3 gives a sum that is a float32 number
    but needs all 24 bits, and the matrix instruction was seen to return other last bits for it when the weight codes are e4m3
    subnormals (test_a_full_width_accumulate_stays_within_the_bound)"""
    for name in names:
        W = np.asarray(sd[name], np.float64)
        s = np.asarray(shifts[name], np.int64)
        top = np.abs(W.reshape(len(W), -1)).max(1)
        assert s.shape == (len(W),) and set(s) == set(range(-2, 3)) and (top > 0).all(), name
        sh = (-1,) + (1,) * (W.ndim - 1)
        sd[name] = (np.rint(3 * W / top.reshape(sh)) / 8 * np.ldexp(1.0, s).reshape(sh)).astype(np.float32)
        b = name[:-len("weight")] + "bias"
        bias = np.asarray(sd[b], np.float64)
        bias = np.rint(bias / BIAS_GRID) * BIAS_GRID if bias_grid else bias
        sd[b] = (bias * np.ldexp(1.0, s)).astype(np.float32)
    return sd


def impulse_sums_fit(W, b, amp, nbits):
    """every conv output of an impulse probe, b[c] + amp W[c, ci, tap], has at most nbits significant bits (24: it is a float32
    number and the probe leaves no rounding to the device; fewer: with bits to spare)"""
    x = np.asarray(b, np.float64).reshape((-1, 1, 1, 1)) + float(amp) * np.asarray(W, np.float64)
    f, ex = np.frexp(x)
    return bool((np.ldexp(np.rint(np.ldexp(f, nbits)), ex - nbits) == x).all())


# ------------------------------------------------------------------ split patterns
def lone_channel(O, k):
    """the one channel that `lone` moves in conv k: one of tower_ref.chan8 (the last real plane of the 73-wide conv)"""
    return tw.chan8(O)[k % 8] if O in (128, 256) else O - 1


def _step_past(lo, hi, start, taken):
    """the first exponent of [lo, hi], counted cyclically from start, that is not in taken (start itself if all are)"""
    w = hi - lo + 1
    for d in range(min(w, len(taken) + 1)):
        c = lo + (start - lo + d) % w
        if c not in taken:
            return c
    return lo + (start - lo) % w


def split(sd, nb, pattern, names=None):
    """-> name -> int8[O]: the channel exponents of every conv in names (None: all of conv_names(nb)) under `pattern`, each inside
    the channel's window; the convs left out keep the canonical exponents (and are not in the result).
      ramp       the exponent of the window congruent to 7n + 3k modulo its width, stepped past the exponent of the row above and of
                 the same row of the conv before: neighbouring rows, and the same row of adjacent convs, all differ
      tiles      one exponent for a 32-channel tile (congruent to 5t + 3k in the tile's common window), stepped past the tile
                 before and the same tile of the conv before; a tile without a common exponent stays canonical
      lone       canonical but for lone_channel, which sits at the top of its window
      subnormal  every channel at the top of its window: the smallest codes that still hold the weights"""
    assert pattern in PATTERNS
    out, prev = {}, None
    for k, name in enumerate(conv_names(nb)):
        W = np.asarray(sd[name], np.float32)
        O = len(W)
        e = scw.channel_exps(W).astype(np.int64)
        if names is None or name in names:
            lo, hi = window(W)
            assert (lo <= hi).all() and (lo <= e).all() and (e <= hi).all(), name
            if pattern == "ramp":
                for n in range(O):
                    taken = ([e[n - 1]] if n else []) + ([prev[n]] if prev is not None and n < len(prev) else [])
                    e[n] = _step_past(lo[n], hi[n], 7 * n + 3 * k, taken)
            elif pattern == "tiles":
                for t in range(-(-O // 32)):
                    s = slice(32 * t, min(32 * t + 32, O))
                    L, H = lo[s].max(), hi[s].min()
                    if L <= H:
                        taken = ([e[32 * t - 1]] if t else []) + ([prev[32 * t]] if prev is not None and 32 * t < len(prev) else [])
                        e[s] = _step_past(L, H, 5 * t + 3 * k, taken)
            elif pattern == "lone":
                e[lone_channel(O, k)] = hi[lone_channel(O, k)]
            else:
                e = hi.copy()
            out[name] = e.astype(np.int8)
        prev = e
    return out


# ------------------------------------------------------------------ the ends of the range
def extremes(sd, name, dead, tiny):
    """-> (state dict, exps): conv `name` with channel `dead` all zero at exponent +100 (its conv output is its bias) and channel
    `tiny` with its codes kept at exponent -100 (weights of about 2^-100: the closed forms take them as they are)"""
    W = np.asarray(sd[name], np.float32).copy()
    e = scw.channel_exps(W).astype(np.int64)
    assert dead != tiny and np.array_equal(scw.quantize_fp8(W)[2], W)
    W[dead] = 0
    W[tiny] = np.ldexp(W[tiny], int(E_MIN - e[tiny]))
    e[dead], e[tiny] = E_MAX, E_MIN
    return dict(sd, **{name: W}), {name: e.astype(np.int8)}


# ------------------------------------------------------------------ what a faulty device would compute
def table(sd, exps, nb):
    """the exponents of the device's scale table [conv][256 = 8 tiles x 32 rows] (pack8 of csrc/weights.hpp writes 127 + e): the
    padded channels of the 73-wide conv hold 0, the tiles a conv does not have are UNWRITTEN"""
    names = conv_names(nb)
    T = np.full((len(names), 256), UNWRITTEN, np.int64)
    for k, name in enumerate(names):
        O = np.shape(sd[name])[0]
        T[k, :-(-O // 128) * 128] = 0
        T[k, :O] = exps[name] if name in exps else scw.channel_exps(sd[name])
    return T


def wrong(sd, exps, nb, name, rule):
    """-> state dict (float64 weights for `name`): what the device computes for conv `name` if the scale of row n is taken
      tile^1          from the same row of the neighbouring tile
      row+1           from row (l + 1) mod 32 of its tile
      next conv       from the table row of conv k + 1 (`san` not swapped in; cyclic at the end of the table)
      previous block  from the table row of conv k - 2 (cyclic)
      negated         as 2^-e
      ignored         as the canonical exponent of scw.channel_exps, whatever the blob says
      upper K half    from row (l + 1) mod 32 for the upper 32 of every 64 input channels (lanes 32..63), its own for the lower"""
    assert rule in RULES
    names = conv_names(nb)
    k, T = names.index(name), table(sd, exps, nb)
    W = np.asarray(sd[name], np.float64)
    n = np.arange(len(W))
    e, nxt = T[k, n], T[k, (n & ~31) | ((n + 1) & 31)]
    sh = (-1,) + (1,) * (W.ndim - 1)
    if rule == "upper K half":
        Wn = W.copy()
        up = np.arange(W.shape[1]) % 64 >= 32
        Wn[:, up] = W[:, up] * np.ldexp(1.0, nxt - e).reshape(sh)
    else:
        used = {"tile^1": T[k, n ^ 32], "row+1": nxt, "next conv": T[(k + 1) % len(names), n], "previous block": T[(k - 2) % len(names), n],
                "negated": -e, "ignored": scw.channel_exps(sd[name]).astype(np.int64)}[rule]
        Wn = W * np.ldexp(1.0, used - e).reshape(sh)
    return dict(sd, **{name: Wn})


# ------------------------------------------------------------------ the nets of the tests (shared by the CPU and the GPU tests)
def block_convs(nb, skip=()):
    return [n for n in conv_names(nb)[1:1 + 2 * nb] if n not in skip]


def coarse_a(C, bias_grid=True):
    """form (a) with five derived exponents in the stem.  Without the bias grid channel 97 keeps its seeded bias of -1.17 2^-19
    (tower_ref.SEED) beside weights of 1/8 to 3/8: its sums are float32 numbers that need all 24 bits"""
    sd = tw.net_a(C, "fp8")
    return coarse(sd, conv_names(1)[:1], draw_shifts(sd, conv_names(1)[:1], SEED), bias_grid)


def coarse_c(C, off, nb=1, blk=0):
    """form (c) in block blk -> (sd, v0, v1): conv2 of that block coarse, and with nb > 1 both convs of every other (transparent)
    block, each with shifts of its own; the stem and conv1 of block blk stay the pass-through convs (weight 1: window [-8, 9])"""
    sd, v0, v1 = tw.net_c(C, "fp8", off, nb=nb, blk=blk)
    names = block_convs(nb, skip=(f"res_blocks.{blk}.conv1.weight",))
    return coarse(sd, names, draw_shifts(sd, names, SEED + 1 + blk)), v0, v1


def heads_net(C, k, nb):
    """heads_ref.net k behind nb transparent blocks whose convs are coarse: every conv of the net has a window to split in"""
    sd = hr.net(C, "fp8", k, nb=nb)
    return coarse(sd, block_convs(nb), draw_shifts(sd, block_convs(nb), SEED + 5))


def dense_net(nb, C):
    """seeded weights with every e4m3 conv coarse: a net for dense inputs (inexact partial sums) whose every channel can be split"""
    sd = tw.natural(nb, C, SEED + 6, "fp8")
    return coarse(sd, conv_names(nb), draw_shifts(sd, conv_names(nb), SEED + 7))


# ------------------------------------------------------------------ the oracle and the engine, passed in
def oracle_latents(orc, sd, nb, C, boards):
    """the fp8-emulating oracle's latent [n][64][C] of the net made of sd's stem, its first nb blocks and its heads"""
    net = orc.Net(nb, C, seed=1, emulate_fp8=True)
    for i, (name, _, _, _) in enumerate(scw.tensor_table(nb, C)):
        net.set_tensor(i, np.asarray(sd[name], np.float32))
    return np.stack([net.forward(b, np.zeros(7, np.int32), latent=True)[2] for b in boards])


def engine_from_split(scamd, tmp_path, sd, exps, nb, C):
    """an fp8 Engine on the weights sd, written as an SCW2 blob with the channel exponents exps (convs not named: canonical) and
    loaded from it; every tensor must be held by its format without loss"""
    for name in conv_names(nb):
        a = np.asarray(sd[name], np.float32)
        assert np.array_equal(scw.quantize_fp8(a, exps.get(name))[2], a), f"{name}: not representable under the given split"
    tw.representable({k: v for k, v in sd.items() if not scw.is_fp8_conv(k)}, "fp8")
    path = str(tmp_path / "w8.scw")
    scw.write_scw(path, sd, nb, C, fp8=True, exps=exps)
    eng = scamd.Engine(n_res_blocks=nb, channels=C, weights=path, precision="fp8")
    assert eng.precision == "fp8" and eng.channels == C
    return eng
