"""The yardstick of the head tests: probe weights that make the operands of every head layer known exactly, float64 closed forms of the
value and of the 4672 log-probabilities that must come out, and the error bounds the oracle and the GPU results are held to.

The heads (csrc/nn_tower32.hpp from "value head conv" to the flatten, the FC1 tiles of csrc/nn_kernels.hpp, the packers of
csrc/weights.hpp) lie between the trunk (tests/tower_ref.py) and the tail (tests/tail_ref.py).  They have no debug output, every head
input passes a LayerNorm, and the policy head has no ReLU behind its LayerNorm, so the trunk suite's lone impulse does not carry over.
This module is plain numpy float64; it imports nothing from the engine or the oracle.

THE BUILDING BLOCK: A SIGN-PATTERN LAYERNORM.  A row of +-1 with as many of each sign, over a power-of-two width, has sum 0 and sum of
squares C exactly in any summation order: ln_reduce (nn_tower32.hpp:306-351) gives mean 0, var 1, rstd = frsqrt(1 + 1e-6) = 1 - 2^-21
(the nearest float), and ln_apply y = +-(1 - 2^-21) g + e.  With the bias e = g 2^-21 the positive side is g itself in plain float32,
and either side lies four orders of magnitude inside the rounding cell of a bf16 or e4m3 value g: the operand the next conv reads is
exactly +-g, or g / 0 behind a ReLU (`_pattern_ln` asserts the margin with tower_ref.tie_margin, TIE_SAFETY bounds wide, for every
element of every row it rounds).

PAIRS.  Channels 2k and 2k+1 of the stem, of the value conv and of the first policy conv form pair k; in every row one member is +1
and the other -1, so behind a ReLU exactly one member of a pair is active.
  * stem: bias s0 = (t, -t), weight -2 s0[o] from ONE board plane rho(k) through ONE tap: the pair shows the plane's bit at the pixel
    (or, through an off-centre tap, at a neighbour; 0 beyond the edge) on ANY 0/1 board; a net uses the centre tap, or both.  LayerNorm gain G[c] in {1/2, 1, 2}, bias
    G[c] 2^-21: the latent is G[c] [sign +].
  * value conv and policy conv1 (1x1, C -> 256): head channel o reads latent pair pi(o // 2) in one of three ways -- (bias 0, weights
    T, -T), (bias -T, weights 2T, 0), (bias T, weights 0, -2T), all over G[c] -- and carries a weight u[o,k] = +-1 (over G[c]) on BOTH
    members of every pair, taken off again by the bias (one member is active: the two add u exactly once).  The two gains of a pair
    differ, so the two weights of a pair differ wherever they are not both 0: the weights are dense, a weight read from the
    neighbouring slot shows, every sum is a sum of small integers and every output row is a balanced +-1 row.
  * several nets differ in the planes, the tap, the pairing pi and the polarities (`nets`).
Everything downstream of the stem is 1x1, so a position's heads depend on its 64 (shifted) board rows one by one: the forms compute
the chain once for every DISTINCT row and gather.

FORMS.
  (v) value: features G'[c] [sign +] in bf16; value_head.ffn.0 with +-1/16 on all 16384 feature columns (all columns distinct), zero
      meta columns, a bias on the 1/4 grid: every partial sum of the K loop is exact in fp32 in any order and under any split-K
      (`_exact`: the sum of the terms' magnitudes stays below 2^24 grid units), h[128] is exact, and from there the value is
      tail_ref.value_closed / value_bound with the feature share (distinct w2[j], |w2| in [3/512, 1/128)).
  (p) policy: Xh = +-G''[o] exactly, conv2 on the 1/8 grid with exact sums, the 73-wide LayerNorm with natural gain and bias
      (tower_ref.ln with the reduction of ln_reduce<1>, K_LN_S73), log-softmax (tail_ref.logp_closed_z / logp_bound_z with the
      LayerNorm's bound carried through), all 4672 actions at ch*64 + px.
The sign patterns have no rounding-tie rows: no form leaves out any row.

BOUNDS, first order in U = 2^-24.  Every head sum up to h and z is exact, so the only bounds are those of the last LayerNorm, the
log-softmax and the value tail.  precision "fp32" is the oracle's mode 0, which rounds no operand: there the pattern LayerNorm is
three float32 operations on known operands (`_pattern_ln`), which the bias g 2^-21 makes exact, so the latent and the features are
the same exact values as in the emulating modes and h is exact again; only the negative side of the policy image stays
-g (1 - 2^-20), and conv2 carries the roundings of the oracle's own sequential sum (oracle/nn.c:239-262: `_seq_err`, one rounding a
product and one a partial sum).  The fp32 bounds stay under the same ceiling as the others."""
import numpy as np

import tail_ref as tr
import tower_ref as tw

U = tr.U
HEAD = 256
# ln_reduce<1> over the 73 policy planes (nn_tower32.hpp:944): the accumulators are 128 wide (4 waves x 32 channels, the padded
# ones exact zeros), so S is summed as at C = 128 -- :313-325 8 registers in two packed halves (7 roundings), a2.x + a2.y (1), :330-332
# the lane^32 add (1), :341-343 the 4-wave pairwise add (2) -- and :337 inv = 1.0f / 73 is itself rounded (k_inv = 1: one more
# rounding in :344 mean and in :345 Q * inv)
K_LN_S73 = 7 + 1 + 1 + 2
G_LATENT = (0.5, 1.0, 2.0)                         # powers of two: the head conv weights k / G[c] stay e4m3
G_VALUE = (1.0, 1.0, 1.0, 2.0)                     # bf16 features; mostly 1 keeps h, and with it the FC2 bound, small
G_POLICY = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)      # e4m3 (and bf16) operands of conv2
LN_BIAS = 2.0 ** -21       # LayerNorm bias g 2^-21: fl(rsqrt(1 + 1e-6)) = 1 - 2^-21, so g (1 - 2^-21) + g 2^-21 is g in plain float32
SEED = 53
BATCHES = (1, 63, 64, 65, 129)
MIN_RATIO = 100            # one grid unit in a single h[j] moves the value by at least this many bounds


def nets(C):
    """(plane offset of the stem pairs, stem tap (ky, kx), pairing offset, pairing step): in the third net every other pair reads a
    neighbour pixel, the others the pixel itself (so that every pixel of a board keeps a pattern of its own)"""
    if C == 128:
        return ((0, (1, 1), 0, 1), (48, (1, 1), 37, 7), (24, (0, 2), 11, 19))
    return ((0, (1, 1), 0, 1), (56, (1, 1), 37, 7), (28, (0, 2), 11, 19))


# ------------------------------------------------------------------ probe nets
def _stem(sd, C, off, tap, rng):
    P = C // 2
    rho = (np.arange(P) + off) % 112
    t = rng.choice([-1.0, 1.0], P)
    s0 = np.stack([t, -t], 1).reshape(C)
    W = np.zeros((C, 112, 3, 3), np.float32)
    near = np.repeat(np.arange(P) % 2 == 1, 2) & (tap != (1, 1))          # a net with an off-centre tap: every other pair reads it
    W[np.arange(C), np.repeat(rho, 2), np.where(near, tap[0], 1), np.where(near, tap[1], 1)] = -2.0 * s0
    G = np.stack([rng.permutation(G_LATENT)[:2] for _ in range(P)]).reshape(C)       # the two members of a pair differ
    sd["conv_block.0.weight"], sd["conv_block.0.bias"] = W, s0.astype(np.float32)
    sd["conv_block.1.weight"], sd["conv_block.1.bias"] = G.astype(np.float32), (G * LN_BIAS).astype(np.float32)
    return G


def pairing(C, pi_off, step):
    """latent pair read by head pair m: at C = 128 two head pairs share a latent pair, and the partner differs from net to net"""
    P, m = C // 2, np.arange(HEAD // 2)
    return (m + pi_off + (m // P) * step) % P


def _pair_conv(sd, name, C, G, pi, rng):
    """in place: 1x1 conv `name` C -> 256 of the module docstring; the LayerNorm behind it is set by the caller"""
    P = C // 2
    T = np.stack([t := rng.choice([-1.0, 1.0], HEAD // 2), -t], 1).reshape(HEAD)
    how = rng.integers(0, 3, HEAD)
    u = rng.choice([-1.0, 1.0], (HEAD, P))
    w = np.repeat(u, 2, axis=1)
    k, o = np.repeat(pi, 2), np.arange(HEAD)
    w[o, 2 * k] += np.choose(how, [T, 2 * T, 0 * T])
    w[o, 2 * k + 1] += np.choose(how, [-T, 0 * T, -2 * T])
    b = np.choose(how, [0 * T, -T, T]) - u.sum(1)
    sd[name + ".weight"] = (w / G[None, :]).astype(np.float32).reshape(HEAD, C, 1, 1)
    sd[name + ".bias"] = b.astype(np.float32)


def head_tensors(C, prec, k, big72=False):
    """-> name -> tensor: the stem and the heads of probe net k (every tensor outside the residual blocks)"""
    off, tap, pi_off, step = nets(C)[k]
    rng = np.random.default_rng(SEED + 10 * k + (C == 256))
    sd = {n: a for n, a in tw.natural(0, C, SEED + k, prec).items()}
    G = _stem(sd, C, off, tap, rng)
    pi = pairing(C, pi_off, step)
    _pair_conv(sd, "value_head.conv.0", C, G, pi, rng)
    sd["value_head.conv.1.weight"] = rng.choice(G_VALUE, HEAD).astype(np.float32)
    sd["value_head.conv.1.bias"] = sd["value_head.conv.1.weight"] * np.float32(LN_BIAS)
    _pair_conv(sd, "policy_head.model.0", C, G, np.roll(pi, 5), rng)
    sd["policy_head.model.1.weight"] = rng.choice(G_POLICY, HEAD).astype(np.float32)
    sd["policy_head.model.1.bias"] = sd["policy_head.model.1.weight"] * np.float32(LN_BIAS)
    W1 = np.zeros((128, 64 * HEAD + 7), np.float32)
    W1[:, :64 * HEAD] = rng.choice([-1.0, 1.0], (128, 64 * HEAD)) / 16.0
    kk = np.arange(192, 256)
    w2 = rng.permutation(np.concatenate([kk, -kk])) / 2.0 ** 15          # 128 distinct bf16 values, |w2| in [3/512, 1/128)
    sd["value_head.ffn.0.weight"], sd["value_head.ffn.0.bias"] = W1, tw.dyadic(rng, 128, -8, 8, 4)
    sd["value_head.ffn.2.weight"], sd["value_head.ffn.2.bias"] = w2.astype(np.float32).reshape(1, 128), np.zeros(1, np.float32)
    sd["policy_head.model.2.weight"], sd["policy_head.model.2.bias"] = tw.dyadic(rng, (73, HEAD, 1, 1), -3, 3, 8), tw.dyadic(rng, 73, -8, 8, 4)
    if big72:       # the last real plane large in both LayerNorm sums: a padded channel that took part would show
        sd["policy_head.model.2.weight"][72] = tw.dyadic(rng, (HEAD, 1, 1), -3, 3, 8)
        sd["policy_head.model.3.weight"][72] *= 8
        sd["policy_head.model.3.bias"][72] = 4.0
    return sd


def net(C, prec, k, nb=1, big72=False):
    """probe net k with nb transparent residual blocks, each with natural weights of its own: the stem and the heads do not depend on nb"""
    sd = tw.natural(nb, C, SEED + 3 + nb, prec)
    sd.update(head_tensors(C, prec, k, big72))
    for b in range(nb):
        tw.transparent_block(sd, C, b)
    tw.representable(sd, prec)
    return sd


# ------------------------------------------------------------------ positions
def impulse_positions():
    """every plane x every pixel: 7168 lone impulses"""
    pl, px = np.repeat(np.arange(112), 64), np.tile(np.arange(64), 112)
    return tw.impulse_board(pl, px)


def random_boards(n, seed=7):
    """multi-impulse boards: every plane bit of every pixel drawn on its own, so that the pixels of a board carry different patterns"""
    return np.random.default_rng(seed).integers(0, 2, (n, 8, 8, 112)).astype(np.int8)


def metas(n):
    """both values of meta[0] (the sign of the value); the other meta columns have zero weights"""
    m = np.zeros((n, 7), np.int32)
    m[:, 0] = (np.arange(n) // 3) % 2
    m[:, 1] = 1 + np.arange(n) % 5
    return m


# ------------------------------------------------------------------ the chain on distinct board rows
def _taps(sd):
    """the taps the probe stem reads, and its weights over the board rows these taps show: [C, taps x 112]"""
    W = np.asarray(sd["conv_block.0.weight"], np.float64)
    taps = [(ky, kx) for ky in range(3) for kx in range(3) if W[:, :, ky, kx].any()]
    return taps, np.concatenate([W[:, :, ky, kx] for ky, kx in taps], axis=1)


def board_rows(sd, boards):
    """-> (rows[R, taps x 112] float64: the distinct board rows the stem's taps show to a pixel (0 beyond the edge), inv[n,64]: which
    of them pixel p of position n sees)"""
    taps, _ = _taps(sd)
    b = np.asarray(boards, np.int8).reshape(-1, 8, 8, 112)
    pad = np.zeros((len(b), 10, 10, 112), np.int8)
    pad[:, 1:9, 1:9] = b
    seen = np.concatenate([pad[:, ky:ky + 8, kx:kx + 8] for ky, kx in taps], axis=-1).reshape(-1, 112 * len(taps))
    key = np.packbits(seen.astype(bool), axis=-1).view(np.dtype((np.void, 14 * len(taps)))).ravel()
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    return seen[first].astype(np.float64), inv.reshape(len(b), 64)


def _exact(label, absum, unit):
    """every partial sum, in any order and under any split, is exact in fp32: the terms are multiples of `unit` (the callers' grids)
    and their magnitudes add up to less than 2^24 units"""
    assert np.array_equal(np.rint(absum / unit), absum / unit) and absum.max() / unit < 2.0 ** 24, label
    return absum.max() / unit


def _seq_err(terms):
    """float32 roundings of a sum taken in the order of the last axis (the oracle): one per product, one per partial sum"""
    return U * (np.abs(np.cumsum(terms, -1)).sum(-1) + np.abs(terms).sum(-1))


def _balanced(label, x):
    assert np.array_equal(np.abs(x), np.ones_like(x)) and not x.sum(-1).any(), f"{label}: no balanced +-1 row"


def _pattern_ln(label, x, g, e, fmt, relu):
    """the operand the next layer reads behind the LayerNorm of balanced +-1 rows x (asserted), exactly.  fmt "bf16" / "fp8": the
    float64 LayerNorm rounded to the format; every element lies TIE_SAFETY bounds from a tie, and from 0 in front of a ReLU
    (asserted).  fmt None (the oracle's fp32 mode, which rounds no operand): mean 0 and variance 1 are exact, rstd =
    (float)(1.0 / sqrt(1 + 1e-6)) is one known float, 1 - 2^-21, and y = (float)(x - m) * rstd * g + e (oracle/nn.c:272-274) is
    three float32 operations on known operands, taken here in IEEE float32: with e = g 2^-21 they are exact and give g"""
    _balanced(label, x)
    if fmt is None:
        rstd = np.float32(1.0 / np.sqrt(1.0 + 1e-6))
        assert float(rstd) == 1.0 - 2.0 ** -21
        y = ((x.astype(np.float32) * rstd) * g.astype(np.float32) + e.astype(np.float32)).astype(np.float64)
        return np.maximum(y, 0) if relu else y
    y, d = tw.ln(x, g, e)
    m = tw.tie_margin(y if relu else np.abs(y), fmt)
    assert (m >= tw.TIE_SAFETY * d).all(), f"{label}: an element within {tw.TIE_SAFETY} bounds of a tie"
    r = np.copysign(tw.r_act(np.abs(y), fmt), y)
    return np.where(y > 0, r, 0.0) if relu else r


def _sum(label, b, x, W, unit, seq=False):
    """b + x W^T for exact rows x[R,K] -> (value, bound): every partial sum exact in any order (asserted) and bound 0, or, with seq,
    the roundings of the oracle's sequential float32 sum"""
    b, W = np.asarray(b, np.float64), np.asarray(W, np.float64).reshape(len(b), -1)
    out = b + x @ W.T
    if not seq:
        _exact(label, np.abs(b) + np.abs(x) @ np.abs(W).T, unit)
        return out, np.zeros_like(out)
    return out, np.stack([_seq_err(np.concatenate([b[:, None], r[None, :] * W], axis=1)) for r in x])


def chain(sd, C, prec, rows):
    """the stem and both heads on distinct board rows[R, taps x 112] -> dict: `lat` the latent, `feat` the value features [R,256] (exact at
    every precision), `y` the 73 logits of the pixel with their bound `dy`, and the rows of +-1 in between (asserted balanced)"""
    f64 = lambda name: np.asarray(sd[name], np.float64)
    fmt = None if prec == "fp32" else prec
    x0 = f64("conv_block.0.bias") + rows @ _taps(sd)[1].T                                   # 0/1 times +-2: exact
    lat = _pattern_ln("stem", x0, f64("conv_block.1.weight"), f64("conv_block.1.bias"), fmt, True)
    assert np.array_equal(lat, f64("conv_block.1.weight") * (x0 > 0))
    xv, _ = _sum("value conv", f64("value_head.conv.0.bias"), lat, sd["value_head.conv.0.weight"], 0.5)
    xp, _ = _sum("policy conv1", f64("policy_head.model.0.bias"), lat, sd["policy_head.model.0.weight"], 0.5)
    feat = _pattern_ln("value conv", xv, f64("value_head.conv.1.weight"), f64("value_head.conv.1.bias"), fmt and "bf16", True)
    assert np.array_equal(feat, f64("value_head.conv.1.weight") * (xv > 0))                 # bf16 at both precisions (pk_bf16)
    xh = _pattern_ln("policy conv1", xp, f64("policy_head.model.1.weight"), f64("policy_head.model.1.bias"), fmt, False)
    # the unrounded negative side of the policy image is -g (1 - 2^-20): conv2's terms leave the 1/32 grid there
    z, dz = _sum("policy conv2", f64("policy_head.model.2.bias"), xh, sd["policy_head.model.2.weight"], 1.0 / 32, seq=fmt is None)
    y, dy = tw.ln(z, f64("policy_head.model.3.weight"), f64("policy_head.model.3.bias"), dz, k_s=K_LN_S73, k_inv=1)
    return dict(x0=x0, lat=lat, xv=xv, feat=feat, xp=xp, xh=xh, z=z, y=y, dy=dy)


# ------------------------------------------------------------------ closed forms
def latent_form(sd, C, prec, boards):
    """what tower_ref.r_act of the residual stream must be, bit for bit: G[c] [sign +], [n,64,C]"""
    rows, inv = board_rows(sd, boards)
    return chain(sd, C, prec, rows)["lat"][inv]


def activity(sd, C, boards):
    """bool [n,16384]: which feature columns (ch*64 + px) are non-zero in each position"""
    rows, inv = board_rows(sd, boards)
    on = chain(sd, C, "bf16", rows)["feat"] > 0
    return on[inv].transpose(0, 2, 1).reshape(len(inv), -1)


def _fc1_share(feat, inv, W1):
    """h share of the feature columns [n,128]: sum over pixels and channels of feat[inv[n,p], c] W1[j, c*64 + p] (float64; exact for
    the dyadic probes).  Large sets go through a table over (pixel, distinct row), small ones through the flat product"""
    Wp = np.asarray(W1, np.float64)[:, :64 * HEAD].reshape(128, HEAD, 64)
    n = len(inv)
    if len(feat) * 4 <= n:
        T = np.ascontiguousarray((feat @ Wp.transpose(1, 0, 2).reshape(HEAD, -1)).reshape(len(feat), 128, 64).transpose(2, 0, 1))
        return sum(T[p][inv[:, p]] for p in range(64))
    out = np.empty((n, 128))
    for s in tw.chunks(n, 512):
        out[s] = feat[inv[s]].transpose(0, 2, 1).reshape(s.stop - s.start, -1) @ Wp.reshape(128, -1).T
    return out


def form_v(sd, C, prec, boards, meta, k_fc2=tr.K_FC2_DEVICE):
    """(v) -> (value[n], bound[n], h share of the features [n,128])"""
    rows, inv = board_rows(sd, boards)
    ch = chain(sd, C, prec, rows)
    W1, b1 = np.asarray(sd["value_head.ffn.0.weight"], np.float64), np.asarray(sd["value_head.ffn.0.bias"], np.float64)
    assert not W1[:, 64 * HEAD:].any()
    h = _fc1_share(ch["feat"], inv, W1)
    assert np.array_equal(np.rint(h * 16), h * 16) and np.array_equal(np.rint(b1 * 16), b1 * 16)
    _exact("FC1", np.abs(b1).max() + np.abs(W1).sum(1) * ch["feat"].max(), 1.0 / 16)          # every feature column at its largest
    p = (np.zeros((128, 7)), b1, np.asarray(sd["value_head.ffn.2.weight"], np.float64).reshape(128), float(sd["value_head.ffn.2.bias"][0]))
    rm = prec != "fp32"
    return tr.value_closed(meta, *p, round_meta=rm, feat=h), tr.value_bound(meta, *p, k_fc2=k_fc2, round_meta=rm, feat=h), h


def unit_ratio(sd, v, bd):
    """the smallest move of the value of form_v when a single h[j] moves by one grid unit (1/16), over its bound
    -> (ratio, largest |FC2 sum|)"""
    w2 = np.abs(np.asarray(sd["value_head.ffn.2.weight"], np.float64)).min()
    s = np.arctanh(np.abs(v))
    moved = np.abs(np.tanh(s + w2 / 16) - np.tanh(s))          # an inactive unit one step above 0 moves it as much
    return float((moved / bd).min()), float(s.max())


def form_p(sd, C, prec, boards):
    """(p) -> (logp[n,4672], bound): action ch*64 + px (the flatten is channel-major)"""
    rows, inv = board_rows(sd, boards)
    ch = chain(sd, C, prec, rows)
    z = ch["y"][inv].transpose(0, 2, 1).reshape(len(inv), -1)
    dz = ch["dy"][inv].transpose(0, 2, 1).reshape(len(inv), -1)
    return np.stack([tr.logp_closed_z(r) for r in z]), np.stack([tr.logp_bound_z(r, d) for r, d in zip(z, dz)])


def distinct_pixel_rows(logp):
    """how many of the 64 pixels of a position have reference rows (73 log-probabilities) of their own: where all do, any pixel
    permutation in the flatten shows"""
    return len({r.tobytes() for r in np.asarray(logp).reshape(73, 64).T})
