"""The yardstick of the tower tests: probe weights that make the input of each trunk layer known exactly, float64 closed forms of what
the layer must then put into the fp32 residual stream, and the error bounds the oracle and the GPU results are held to.

The trunk (csrc/nn_tower32.hpp: stem conv, the two 3x3 convs of every residual block, their LayerNorms, squeeze-excitation) is where
almost all simulation time goes.  This module is plain numpy float64; it imports nothing from the engine or the oracle.

WHAT THE DEVICE GIVES (checked in the code):
  * `Engine.debug(boards, meta, stage)` (sc_forward_debug) returns the fp32 residual stream [n][64][C], pixel = rank*8 + file; stage 0
    is after the stem, stage b after the b-th block (1-based), stage 1000 the latent.  It runs the stand-alone k_tower32; the fused
    k_step has no debug output and is held to k_tower32 bit for bit by the fused-step against two-launch tests.  Batches stay within
    sc_engine_max_batch.
  * boards are raw int8 planes, converted exactly: any 0/1 pattern may be passed.  The stem pads K from 112 to 128 per tap.
  * Rounding points (oracle/nn.c modes 1 and 2 restate them): conv operands are bf16, or e4m3 in fp8 mode, where weights carry one
    power-of-two scale per output channel (tools/scw.py: quantize_fp8, e4m3_round, is_fp8_conv) and activations are clamped to +-448
    before the conversion.  The SE pool and hidden vectors are bf16; the SE weights are bf16 at both precisions.  Accumulators,
    LayerNorm, the residual stream and the SE scales are fp32.
  * LayerNorm (ln_reduce / ln_apply), all fp32, one pass: var = Q/C - mean^2 clamped at 0, rstd = __frsqrt_rn(var + 1e-6f),
    y = (x rstd + (-mean rstd)) g + e; S and Q are summed in-lane, then one lane^32 add, then a 4-wave pairwise add.
  * Block output relu(acc scale + res); SE scale rcp(1 + __expf(-(s + b2))); the pool is a butterfly sum times 1/64; the fc1 bias is
    added after the matrix product.

PROBES.  Two kinds, neither depends on a summation order.  IMPULSE probes put one non-zero operand into a conv: every output is one
exact product plus the bias (one accumulator rounding, taken at 1 ulp: MMA_ULP), so a weight read from the wrong tap, channel or pixel
shows at full size.  EXACT-SUM probes draw operands from small dyadic grids: every partial sum of the K loop is exact in fp32 in any
order, so a k-step skipped, doubled or fed a stale fragment moves the result by whole grid units.  Building blocks:
  * pass-through conv + LN: weight `a` on the centre tap from channel ci to sigma(ci), zero bias, LN gain g, bias 0.  A lone impulse
    leaves, after LN and ReLU, a lone impulse v = g (a - a/C) rstd; the other channels of its pixel come out negative (asserted) and
    ReLU clears them; pixels with x = 0 stay exactly 0.  g is chosen so that v is far from a bf16 and an e4m3 tie (asserted).
  * transparent SE: fc2 weights and bias zero, scale = rcp(2), taken as 0.5 within the bound.
  * transparent block: second LayerNorm gain 0, bias 0: acc = 0 and the output is relu(0 s + res) = res.
  * constant layer: LayerNorm gain 0 and bias k[c]: output k[c] at every pixel for every input, exactly.
Every probe value is representable in the engine's operand format (`representable` asserts it), so nothing depends on the loader.

THE ONE ROUNDING ON A DENSE ROW.  Forms (d) and (e)-conv1 round LN1's dense output before conv2.  An element whose float64 value lies
within its LN1 bound of a rounding tie may round the other way on the device, and then the whole LN2 row moves.  The row behind an
impulse depends on (input channel, tap) alone, not on the pixel, so leaving such rows out would drop whole (channel, tap) pairs (13 %
of them at C = 128, 32 % at C = 256 in bf16).  Instead a row with up to MAX_FLIPS such elements is held to the nearest of its
2^MAX_FLIPS rounding variants -- the device must match one of them within the bound -- and only rows with more are left out (none
on the tests' sets; tests/test_tower_ref.py asserts at most 25 % and that every (input channel, tap) pair keeps a compared row).

BOUNDS, first order in U = 2^-24, computed from the data, one term per rounding (the constants below cite their lines).  The one-pass
variance carries its cancellation term (roundings of Q/C and mean^2 against their difference) through rstd; `__expf` is
tail_ref.exp_rel, `rcp` one 2^-23 term.

TWO YARDSTICKS IN `ln`.  Its VALUE is the float64 two-pass LayerNorm, the operation of the reference (F.layer_norm) and of the oracle;
its BOUND models the engine's one-pass fp32 formula, so it grows with (mean / sigma)^2 as that formula's error does and never fails
on a large common offset by itself.  Every form of this module, of heads_ref and of rounding_ref keeps mean / sigma below a few, where
the two coincide.  tests/ln_offset_ref.py takes them apart on rows with mean / sigma up to 32768: its assertion 1 (finite, no worse
than the one-pass formula) uses the bound, its assertion 2 (the operation itself, up to the required ratio R_REQ) uses the value with
a tolerance taken from the operand formats, not from this model."""
import numpy as np

import scw
import tail_ref as tr

U = tr.U
EPS = float(np.float32(1e-6))
MMA_ULP = 2 * U            # conv_mma32: bias (acc_init) + one exact product, one rounding inside the matrix instruction, taken at 1 ulp
# ln_reduce: a2 += v over 16 CT registers in two packed halves (8 CT - 1 roundings a half), a2.x + a2.y, the lane^32 add, the
# 4-wave pairwise add (2 levels)
K_LN_S = lambda C: (8 * (C // 128) - 1) + 1 + 1 + 2    # noqa: E731
K_LN_Q = lambda C: K_LN_S(C) + 1       # noqa: E731  b2 = v * v + b2: the square's rounding on top (an fma has none: upper bound)
K_MEAN = 1                 # ln_reduce: mean = S * inv
K_VAR = 3                  # ln_reduce: Q * inv, mean * mean, their difference
K_RSTD = 2                 # ln_reduce: var + 1e-6f, __frsqrt_rn
K_NM = 1                   # ln_reduce: -mean * rstd
K_APPLY_T = 2              # ln_apply: x * rstd, + nm
K_APPLY_Y = 2              # ln_apply: t * g, + e
K_EPI = 2                  # block epilogue: acc * scale, + res
RCP_REL = 2.0 ** -23       # __builtin_amdgcn_rcpf: 1 ulp
K_SCALE_ADD = 1            # 1.0f + __expf(..)
CEIL = 1e-4                # of the row's largest |reference|: a single wrong bf16 weight moves an element by >= 2^-9 relative
TIE_SAFETY = 100           # an impulse amplitude lies at least this many bounds from a rounding tie
PIX6 = (0, 7, 56, 63, 27, 4)           # a1, h1, a8, h8, d4, e1 (pixel = rank*8 + file)
PRECS = ("bf16", "fp8")


# ------------------------------------------------------------------ operand formats
def r_act(x, prec):
    """the conv-input rounding: float32, then bf16 (ties to even) or e4m3 after the +-448 clamp; float64 in, float64 out"""
    x32 = np.asarray(x, np.float64).astype(np.float32)
    return (tr.bf16_rne(x32) if prec == "bf16" else scw.e4m3_round(np.clip(x32, -448, 448))).astype(np.float64)


def q_w(W, prec):
    """the conv-weight rounding of the engine: bf16, or e4m3 with one power-of-two scale per output channel"""
    W = np.asarray(W, np.float32)
    return tr.bf16_rne(W) if prec == "bf16" else scw.quantize_fp8(W)[2]


def representable(sd, prec, skip=()):
    """assert: every tensor of sd is bf16, and every e4m3 conv weight survives quantize_fp8 unchanged at fp8.  skip: names left out --
    per-channel fp32 parameters that a probe net sets to any float32 (tests/rounding_ref.py: the device keeps them in fp32), and
    tensors that the caller has checked already on the same arrays"""
    for name, a in sd.items():
        if name in skip:
            continue
        a = np.asarray(a, np.float32)
        if prec == "fp8" and scw.is_fp8_conv(name):
            assert np.array_equal(scw.quantize_fp8(a)[2], a), f"{name}: not representable in scaled e4m3"
        else:
            tr._assert_bf16(name, a)


def tie_margin(y, prec):
    """distance of each pre-ReLU value y to the nearest point where relu-then-round changes its result discontinuously: for y <= 0
    that is 0 itself (|y|), for y > 0 the nearer midpoint between the two neighbours of r(y) (in a relative format the midpoints
    crowd towards 0, so small positive values have small margins)"""
    y = np.asarray(y, np.float64)
    a = np.abs(y)
    ry = r_act(a, prec)
    _, ex = np.frexp(np.where(ry > 0, ry, 1.0))
    if prec == "bf16":
        q = np.ldexp(1.0, ex - 1 - 7)
        pow2 = np.ldexp(1.0, ex - 1) == ry
    else:
        q = np.where(ry >= 2.0 ** -6, np.ldexp(1.0, ex - 1 - 3), 2.0 ** -9)
        pow2 = (np.ldexp(1.0, ex - 1) == ry) & (ry > 2.0 ** -6)
    up, dn = ry + q / 2, ry - np.where(pow2, q / 4, q / 2)
    m = np.minimum(np.abs(up - a), np.abs(a - dn))
    if prec == "fp8":
        m = np.where(a >= 448, np.inf, m)     # clamped: no tie above the maximum
        m = np.where(ry == 0, 2.0 ** -10 - a, m)
    else:
        m = np.where(ry == 0, 0.0, m)
    return np.where(y <= 0, a, m)


# ------------------------------------------------------------------ LayerNorm, block epilogue: float64 value and fp32 bound
def ln(x, g, e, dx=0.0, k_s=None, k_inv=0):
    """LayerNorm over the last axis (eps 1e-6), no ReLU: -> (y, bound on |device y - y|) for exact input x whose device copy is off by
    at most dx (elementwise).  k_s: the roundings of the sum S where the width is no multiple of 128 (K_LN_S otherwise); k_inv: 1
    where 1 / width is itself rounded (no power of two): one more rounding in the mean and in Q / C"""
    x = np.asarray(x, np.float64)
    C = x.shape[-1]
    k_s, k_q = (K_LN_S(C), K_LN_Q(C)) if k_s is None else (k_s, k_s + 1)      # Q: the square's rounding on top
    dx = np.broadcast_to(np.asarray(dx, np.float64), x.shape)
    ax = np.abs(x)
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    q = (x * x).mean(-1, keepdims=True)                       # Q / C
    d_mean = (k_s * U * ax.sum(-1, keepdims=True) + dx.sum(-1, keepdims=True)) / C + (K_MEAN + k_inv) * U * np.abs(mean)
    d_q = k_q * U * q + 2 * (ax * dx).mean(-1, keepdims=True)
    # the cancellation term: every rounding of Q/C and of mean^2 is relative to those, not to their difference
    d_var = d_q + 2 * np.abs(mean) * d_mean + (K_VAR + k_inv) * U * (q + mean * mean)
    v = var + EPS
    rstd = v ** -0.5
    rel_rstd = 0.5 * (d_var + U * v) / v + (K_RSTD - 1) * U
    d_nm = rstd * d_mean + np.abs(mean) * rstd * (rel_rstd + K_NM * U)
    t = (x - mean) * rstd
    d_t = ax * rstd * (rel_rstd + U) + rstd * dx + d_nm + (K_APPLY_T - 1) * U * np.abs(t)
    y = t * g + e
    d_y = np.abs(g) * d_t + U * np.abs(t * g) + (K_APPLY_Y - 1) * U * np.abs(y)
    return y, d_y


def scale_of(z):
    """SE scale 1 / (1 + exp(-z)) for an exact fp32 argument z -> (s, bound)"""
    z = np.asarray(z, np.float64)
    E = np.exp(-z)
    s = 1.0 / (1.0 + E)
    return s, s * (E / (1.0 + E) * tr.exp_rel(z) + K_SCALE_ADD * U + RCP_REL)


def epilogue(acc, d_acc, s, d_s, res, d_res):
    """relu(acc s + res) -> (y, bound)"""
    pre = acc * s + res
    d = np.abs(s) * d_acc + np.abs(acc) * d_s + U * np.abs(acc * s) + (K_EPI - 1) * U * np.abs(pre) + d_res
    return np.maximum(pre, 0.0), d


HALF = scale_of(0.0)       # the transparent SE


# ------------------------------------------------------------------ probe nets
def sigmas(C):
    """offsets o of the stem maps sigma(ci) = ci + o that together reach every trunk channel"""
    return (0, 16) if C == 128 else (0, 112, 144)


def chan8(C):
    """8 channels that meet every wave, channel tile, register quad, lane half (chan32 of nn_tower32.hpp) and, at C = 128, every
    K-16 group"""
    off = (0, 5, 10, 15, 3, 6, 9, 12) if C == 128 else (0, 21, 10, 31, 3, 22, 9, 28)
    return tuple((C // 8) * k + off[k] for k in range(8))


PLANES8 = (0, 17, 34, 51, 61, 78, 95, 111)


def natural(nb, C, seed, prec):
    """seed-init weights made representable: e4m3 convs through quantize_fp8 at fp8, everything else through bf16"""
    sd = scw.prng_state_dict(nb, C, seed)
    for name in sd:
        sd[name] = q_w(sd[name], prec) if (prec == "fp8" and scw.is_fp8_conv(name)) else tr.bf16_rne(sd[name])
    return sd


def _gain_far_from_ties(C, amp):
    """-> (g, {prec: (v, bound)}): the first LN gain on the 1/64 grid in [0.5, 1.5) whose impulse v = LN(amp one-hot) g lies
    TIE_SAFETY bounds and an eighth of a spacing from every bf16 and e4m3 tie, for the amplitudes amp[prec]"""
    for k in range(64):
        g = 0.5 + k / 64.0
        out, ok = {}, True
        for prec in PRECS:
            row = np.zeros(C)
            row[0] = amp[prec]
            y, d = ln(row, g, 0.0)
            assert (y[1:] + d[1:] < 0).all()                  # the other channels of the pixel: negative beyond the bound
            m = tie_margin(y[0], prec)
            spacing = 2.0 ** (np.floor(np.log2(y[0])) - (7 if prec == "bf16" else 3))
            ok &= bool(m >= TIE_SAFETY * d[0] and m >= spacing / 8 and y[0] < 400)
            out[prec] = (float(y[0]), float(d[0]))
        if ok:
            return g, out
    raise AssertionError("no gain keeps the impulse clear of a tie")


def passthrough_stem(sd, C, off):
    """in place: stem = centre-tap weight 1 from plane ci to channel ci + off, zero bias, LN gain G0, bias 0 -> (v0, bound) by prec"""
    g, v = _gain_far_from_ties(C, {p: 1.0 for p in PRECS})
    W = np.zeros((C, 112, 3, 3), np.float32)
    W[np.arange(112) + off, np.arange(112), 1, 1] = 1.0
    sd["conv_block.0.weight"], sd["conv_block.0.bias"] = W, np.zeros(C, np.float32)
    sd["conv_block.1.weight"], sd["conv_block.1.bias"] = np.full(C, g, np.float32), np.zeros(C, np.float32)
    return v


def passthrough_conv1(sd, C, blk, v0):
    """in place: conv1 of block blk = centre-tap identity, zero bias, LN1 gain g1, bias 0 -> (v1, bound) by prec; the bound carries v0's"""
    p = f"res_blocks.{blk}."
    g, _ = _gain_far_from_ties(C, {pr: float(r_act(v0[pr][0], pr)) for pr in PRECS})
    sd[p + "conv1.weight"], sd[p + "conv1.bias"] = identity_conv(C), np.zeros(C, np.float32)
    sd[p + "bn1.weight"], sd[p + "bn1.bias"] = np.full(C, g, np.float32), np.zeros(C, np.float32)
    out = {}
    for pr in PRECS:
        assert tie_margin(v0[pr][0], pr) >= TIE_SAFETY * v0[pr][1]
        row = np.zeros(C)
        row[0] = r_act(v0[pr][0], pr)
        y, d = ln(row, g, 0.0)
        out[pr] = (float(y[0]), float(d[0]))
    return out


def identity_conv(C):
    W = np.zeros((C, C, 3, 3), np.float32)
    W[np.arange(C), np.arange(C), 1, 1] = 1.0
    return W


def transparent_se(sd, C, blk):
    p = f"res_blocks.{blk}.se."
    sd[p + "fc2.weight"], sd[p + "fc2.bias"] = np.zeros((C, C // 2, 1, 1), np.float32), np.zeros(C, np.float32)


def transparent_block(sd, C, blk):
    p = f"res_blocks.{blk}."
    sd[p + "bn2.weight"], sd[p + "bn2.bias"] = np.zeros(C, np.float32), np.zeros(C, np.float32)


def constant_layer(sd, prefix, k):
    """LayerNorm `prefix`: gain 0, bias k[c]"""
    k = np.asarray(k, np.float32)
    sd[prefix + ".weight"], sd[prefix + ".bias"] = np.zeros_like(k), k


def dyadic(rng, shape, lo, hi, den):
    return (rng.integers(lo, hi + 1, shape) / float(den)).astype(np.float32)


def kappa(C, seed):
    """a constant stem output: multiples of 1/4 in [0, 1.75] (3 significant bits: bf16 and e4m3), a few of them 0"""
    return dyadic(np.random.default_rng(seed), C, 0, 7, 4)


# ------------------------------------------------------------------ positions
def impulse_board(planes, pixels):
    planes, pixels = np.asarray(planes), np.asarray(pixels)
    b = np.zeros((len(planes), 64, 112), np.int8)
    b[np.arange(len(planes)), pixels, planes] = 1
    return b.reshape(-1, 8, 8, 112)


def impulse_set(chans_all_pixels, chans_six):
    """-> (channel[n], pixel[n]): every pixel for the first list, PIX6 for the second"""
    six = [c for c in chans_six if c not in chans_all_pixels]
    c = [c for c in chans_all_pixels for _ in range(64)] + [c for c in six for _ in PIX6]
    p = [p for _ in chans_all_pixels for p in range(64)] + [p for _ in six for p in PIX6]
    return np.asarray(c, np.int64), np.asarray(p, np.int64)


def neighbours(pix):
    """-> out[n,9] (output pixel that reads the impulse at pix through tap ky*3+kx, -1 off the board)"""
    r0, f0 = pix[:, None] // 8, pix[:, None] % 8
    ky, kx = np.arange(9)[None, :] // 3, np.arange(9)[None, :] % 3
    r, f = r0 - ky + 1, f0 - kx + 1
    return np.where((r >= 0) & (r < 8) & (f >= 0) & (f < 8), r * 8 + f, -1)


def impulse_rows(W, b, cin, amp):
    """conv outputs of a lone impulse amp at input channel cin[n]: rows[n,9,C] = b + amp W[:, cin, tap] (exact), and their device error"""
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
    rows = b[None, None, :] + amp * W[:, cin].reshape(W.shape[0], len(cin), 9).transpose(1, 2, 0)
    return rows, MMA_ULP * np.abs(rows)


def expand(base, rows, out):
    """[C] base row, rows[n,9,C] at output pixels out[n,9] -> [n,64,C]"""
    n, C = rows.shape[0], rows.shape[-1]
    full = np.broadcast_to(base, (n, 64, C)).copy()
    i, t = np.nonzero(out >= 0)
    full[i, out[i, t]] = rows[i, t]
    return full


def add_impulse(full, chan, pix, v):
    full[np.arange(len(chan)), pix, chan] += v
    return full


# ------------------------------------------------------------------ closed forms
def form_a(sd, prec, planes, pix):
    """(a) stem, impulse: stage 0 of a board that is a single 1 at (plane, pixel) under natural stem weights"""
    W, b = sd["conv_block.0.weight"], sd["conv_block.0.bias"]
    g, e = np.float64(sd["conv_block.1.weight"]), np.float64(sd["conv_block.1.bias"])
    rows, dx = impulse_rows(W, b, planes, 1.0)
    y, d = ln(rows, g, e, dx)
    y0, d0 = ln(np.float64(b), g, e)
    out = neighbours(pix)
    return np.maximum(expand(y0, y, out), 0), expand(d0, d, out)


def conv_exact(x, W, b):
    """dense 3x3 conv, zero padding: x[n,64,Cin], W[Cout,Cin,3,3] -> [n,64,Cout] in float64 (exact for the dyadic probes)"""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    n, _, cin = x.shape
    xp = np.zeros((n, 10, 10, cin))
    xp[:, 1:9, 1:9] = x.reshape(n, 8, 8, cin)
    out = np.broadcast_to(np.asarray(b, np.float64), (n, 8, 8, W.shape[0])).copy()
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + 8, kx:kx + 8] @ W[:, :, ky, kx].T
    return out.reshape(n, 64, -1)


def sums_are_exact(x, W, b, pixels):
    """the terms of conv_exact at the given output pixels of position 0, summed in float32 forwards, backwards and pairwise, equal
    the float64 sum bit for bit"""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    cin = x.shape[-1]
    xp = np.zeros((10, 10, cin))
    xp[1:9, 1:9] = x[0].reshape(8, 8, cin)
    for p in pixels:
        patch = xp[p // 8:p // 8 + 3, p % 8:p % 8 + 3]                                        # [ky][kx][cin]
        terms = np.concatenate([np.asarray(b, np.float64)[:, None],
                                (W.transpose(0, 2, 3, 1) * patch[None]).reshape(W.shape[0], -1)], axis=1)
        _exact_orders(terms)
    return True


def _exact_orders(terms):
    """terms[rows, K] float64: float32 sums in three orders equal the float64 sum"""
    t32 = terms.astype(np.float32)
    assert np.array_equal(t32.astype(np.float64), terms)
    ref = terms.sum(-1)
    fwd = np.cumsum(t32, axis=-1, dtype=np.float32)[:, -1]
    rev = np.cumsum(t32[:, ::-1], axis=-1, dtype=np.float32)[:, -1]
    pw = t32.copy()
    while pw.shape[1] > 1:
        if pw.shape[1] % 2:
            pw = np.concatenate([pw, np.zeros((pw.shape[0], 1), np.float32)], axis=1)
        pw = pw[:, 0::2] + pw[:, 1::2]
    for s in (fwd, rev, pw[:, 0]):
        assert np.array_equal(s.astype(np.float64), ref), "a float32 partial sum is inexact"


def stem_grid(sd, C, seed):
    """in place: stem weights on the 1/8 grid in [-3/8, 3/8], bias on the 1/4 grid: every partial sum over 9 x 112 planes is exact"""
    r = np.random.default_rng(seed)
    sd["conv_block.0.weight"], sd["conv_block.0.bias"] = dyadic(r, (C, 112, 3, 3), -3, 3, 8), dyadic(r, C, -8, 8, 4)


def form_b(sd, boards):
    """(b) stem, exact sums: stage 0 of dense boards under grid stem weights"""
    x = conv_exact(np.asarray(boards, np.float64).reshape(len(boards), 64, 112), sd["conv_block.0.weight"], sd["conv_block.0.bias"])
    y, d = ln(x, np.float64(sd["conv_block.1.weight"]), np.float64(sd["conv_block.1.bias"]))
    return np.maximum(y, 0), d


def x0_impulse(n, C, chan, pix, v0):
    x0, d0 = np.zeros((n, 64, C)), np.zeros((n, 64, C))
    return add_impulse(x0, chan, pix, v0[0]), add_impulse(d0, chan, pix, v0[1])


def form_c(sd, prec, blk, chan, pix, v0, v1):
    """(c) conv2, impulse: stage blk+1 = relu(0.5 LN2(b2 + r(v1) W2[:, c0, tap]) + x0) behind a pass-through stem and conv1"""
    p = f"res_blocks.{blk}."
    assert tie_margin(v1[0], prec) >= TIE_SAFETY * v1[1]
    rows, dx = impulse_rows(sd[p + "conv2.weight"], sd[p + "conv2.bias"], chan, float(r_act(v1[0], prec)))
    g, e = np.float64(sd[p + "bn2.weight"]), np.float64(sd[p + "bn2.bias"])
    y, d = ln(rows, g, e, dx)
    yb, db = ln(np.float64(sd[p + "conv2.bias"]), g, e)
    out = neighbours(pix)
    x0, d0 = x0_impulse(len(chan), len(g), chan, pix, v0)
    return epilogue(expand(yb, y, out), expand(db, d, out), HALF[0], HALF[1], x0, d0)


MAX_FLIPS = 4              # a row with more elements than this on a rounding tie is left out; up to it, both roundings are tried


def round_rows(y1, d1, prec):
    """the conv input r(relu(y1)) when the device's y1 is only known to d1: -> (value, input error, flip mask, other value).  The
    device's operand lies between lo = r(relu(y1 - d1)) and hi = r(relu(y1 + d1)).  Where they agree it is known.  Where they
    differ by no more than 8 d1 (near 0 the bf16 grid is finer than the error) it is the reference's own rounding to within hi - lo,
    an input error of the next layer.  Elsewhere the interval holds exactly one tie and the operand is one of two neighbours: the
    reference's own or the other"""
    lo, hi = r_act(np.maximum(y1 - d1, 0), prec), r_act(np.maximum(y1 + d1, 0), prec)
    base = r_act(np.maximum(y1, 0), prec)
    flip = (hi != lo) & (hi - lo > 8 * d1)
    return base, np.where((hi != lo) & ~flip, hi - lo, 0.0), flip, np.where(base == lo, hi, lo)


def _variants(base, dx2, flip, alt, g2, e2):
    """rows[m,C] with 1..MAX_FLIPS flips each -> LN2 of the 2^MAX_FLIPS operand rows [m,V,C] (rows with fewer flips repeat variants)"""
    m = len(base)
    j = np.argsort(~flip, axis=-1, kind="stable")[:, :MAX_FLIPS]
    ok = np.take_along_axis(flip, j, -1)
    X = np.repeat(base[:, None, :], 2 ** MAX_FLIPS, 1)
    for k in range(MAX_FLIPS):
        for v in range(2 ** MAX_FLIPS):
            if v >> k & 1:
                rows = np.flatnonzero(ok[:, k])
                X[rows, v, j[rows, k]] = alt[rows, j[rows, k]]
    return ln(X, g2, e2, dx2[:, None, :])


def form_d(sd, prec, blk, chan, pix, v0):
    """(d) conv1, impulse: stage blk+1 = relu(0.5 LN2(r(relu(LN1(b1 + r(v0) W1[:, c0, tap])))) + x0), conv2 the centre-tap identity
    -> (reference, bound, keep[n,64], alts).  The one rounding point on a dense row: an element whose float64 value lies within its
    LN1 bound of a rounding tie may round the other way on the device, and the whole LayerNorm row moves with it.  keep marks the
    rows without such an element; alts = (position, pixel, reference[m,V,C], bound[m,V,C]) holds the rows with 1..MAX_FLIPS of them
    under every combination of roundings (the device must match one); rows with more are left out"""
    p = f"res_blocks.{blk}."
    assert tie_margin(v0[0], prec) >= TIE_SAFETY * v0[1]
    g1, e1 = np.float64(sd[p + "bn1.weight"]), np.float64(sd[p + "bn1.bias"])
    g2, e2 = np.float64(sd[p + "bn2.weight"]), np.float64(sd[p + "bn2.bias"])
    rows, dx = impulse_rows(sd[p + "conv1.weight"], sd[p + "conv1.bias"], chan, float(r_act(v0[0], prec)))
    out = neighbours(pix)
    n, C = len(chan), len(g1)
    y1, d1 = ln(rows, g1, e1, dx)
    base, dx2, flip, alt = round_rows(y1, d1, prec)
    y, d = ln(base, g2, e2, dx2)                               # identity conv2: exact
    yb1, db1 = ln(np.float64(sd[p + "conv1.bias"]), g1, e1)
    bbase, bdx2, bflip, _ = round_rows(yb1, db1, prec)
    assert not bflip.any(), "the bias row (every pixel away from the impulse) sits on a tie: take another seed"
    yb, db = ln(bbase, g2, e2, bdx2)
    keep = np.ones((n, 64), bool)
    i, t = np.nonzero(out >= 0)
    nf = flip.sum(-1)
    keep[i, out[i, t]] = nf[i, t] == 0
    x0, d0 = x0_impulse(n, C, chan, pix, v0)
    ref, bd = epilogue(expand(yb, y, out), expand(db, d, out), HALF[0], HALF[1], x0, d0)
    sel = (nf[i, t] > 0) & (nf[i, t] <= MAX_FLIPS)
    ai, at = i[sel], t[sel]
    yv, dv = _variants(base[ai, at], dx2[ai, at], flip[ai, at], alt[ai, at], g2, e2)
    apix = out[ai, at]
    rv, bv = epilogue(yv, dv, HALF[0], HALF[1], x0[ai, apix][:, None, :], d0[ai, apix][:, None, :])
    return ref, bd, keep, (ai, apix, rv, bv)


def conv_grid(sd, C, name, seed):
    """in place: conv `name` on the 1/8 grid in [-3/8, 3/8], bias on the 1/4 grid: with inputs on the 1/4 grid up to 1.75 every
    partial sum over 9 C terms is a multiple of 1/32 below 2^24 / 32"""
    r = np.random.default_rng(seed)
    sd[name + ".weight"], sd[name + ".bias"] = dyadic(r, (C, C, 3, 3), -3, 3, 8), dyadic(r, C, -8, 8, 4)


def form_e2(sd, blk, kap, kap1):
    """(e) conv2, exact sums: stem output kap[c] >= 0, LN1 the constant layer kap1[c] >= 0, grid conv2, natural LN2, transparent
    SE -> stage blk+1 [64][C] (the same for every input)"""
    p = f"res_blocks.{blk}."
    x = conv_exact(np.broadcast_to(np.float64(kap1), (1, 64, len(kap1))), sd[p + "conv2.weight"], sd[p + "conv2.bias"])
    y, d = ln(x, np.float64(sd[p + "bn2.weight"]), np.float64(sd[p + "bn2.bias"]))
    ref, bd = epilogue(y, d, HALF[0], HALF[1], np.float64(kap)[None, None, :], 0.0)
    return ref[0], bd[0]


def form_e1(sd, prec, blk, kap):
    """(e) conv1, exact sums: stem output kap[c] >= 0, grid conv1, natural LN1, identity conv2, natural LN2, transparent SE
    -> (stage blk+1 [64][C], bound, keep[64], alts): the rounding behind LN1 is treated as in form_d"""
    p = f"res_blocks.{blk}."
    g2, e2 = np.float64(sd[p + "bn2.weight"]), np.float64(sd[p + "bn2.bias"])
    x = conv_exact(np.broadcast_to(np.float64(kap), (1, 64, len(kap))), sd[p + "conv1.weight"], sd[p + "conv1.bias"])[0]
    y1, d1 = ln(x, np.float64(sd[p + "bn1.weight"]), np.float64(sd[p + "bn1.bias"]))
    base, dx2, flip, alt = round_rows(y1, d1, prec)
    y2, d2 = ln(base, g2, e2, dx2)
    ref, bd = epilogue(y2, d2, HALF[0], HALF[1], np.float64(kap)[None, :], 0.0)
    nf = flip.sum(-1)
    ap = np.flatnonzero((nf > 0) & (nf <= MAX_FLIPS))
    yv, dv = _variants(base[ap], dx2[ap], flip[ap], alt[ap], g2, e2)
    rv, bv = epilogue(yv, dv, HALF[0], HALF[1], np.float64(kap)[None, None, :], 0.0)
    return ref, bd, nf == 0, (np.zeros(len(ap), np.int64), ap, rv, bv)


def se_probe(sd, C, blk, beta, seed):
    """in place: LN2 of block blk the constant layer beta[c]; SE fc1 with 8 weights of +-1/2 a row and a bias on the 1/4 grid, fc2
    with 8 weights of +-1/4, +-1/2 a row and a bias that puts channel c into regime c % 8: near 0, moderate, saturated (|z| >= 40)"""
    r = np.random.default_rng(seed)
    p = f"res_blocks.{blk}."
    constant_layer(sd, p + "bn2", beta)
    W1 = np.zeros((C // 2, C), np.float32)
    W2 = np.zeros((C, C // 2), np.float32)
    for j in range(C // 2):
        W1[j, r.permutation(C)[:8]] = r.choice([-0.5, 0.5], 8)
    for c in range(C):
        W2[c, r.permutation(C // 2)[:8]] = r.choice([-0.5, -0.25, 0.25, 0.5], 8)
    base = np.asarray([0.0, 0.25, -2.0, 3.0, -48.0, 48.0, -8.0, 8.0], np.float32)
    sd[p + "se.fc1.weight"], sd[p + "se.fc1.bias"] = W1.reshape(C // 2, C, 1, 1), dyadic(r, C // 2, -4, 4, 4)
    sd[p + "se.fc2.weight"], sd[p + "se.fc2.bias"] = W2.reshape(C, C // 2, 1, 1), base[np.arange(C) % 8]


def betas(C):
    """name -> beta[c], multiples of 1/4 with both signs (the pool average of a constant is the constant, exact in bf16)"""
    r = np.random.default_rng(21)
    return {"mixed": dyadic(r, C, -8, 8, 4), "positive": dyadic(r, C, 0, 8, 4), "negative": dyadic(r, C, -8, 0, 4)}


def form_f(sd, blk, kap, beta):
    """(f) SE, exact sums: stage blk+1 = relu(beta sigma(z) + kap), z = fc2(bf16(relu(fc1(beta) + b1))) + b2 -> (ref [C], bound, hidden, z)"""
    p = f"res_blocks.{blk}.se."
    C = len(beta)
    W1, b1 = np.float64(sd[p + "fc1.weight"]).reshape(C // 2, C), np.float64(sd[p + "fc1.bias"])
    W2, b2 = np.float64(sd[p + "fc2.weight"]).reshape(C, C // 2), np.float64(sd[p + "fc2.bias"])
    beta = np.float64(beta)
    _exact_orders(np.repeat(beta[:, None], 64, 1))            # the pool: 64 equal terms a channel
    t1 = np.concatenate([W1 * beta[None, :], b1[:, None]], axis=1)
    _exact_orders(t1)
    hid = np.maximum(t1.sum(-1), 0)
    tr._assert_bf16("SE hidden", hid)
    t2 = np.concatenate([W2 * hid[None, :], b2[:, None]], axis=1)
    _exact_orders(t2)
    z = t2.sum(-1)
    s, ds = scale_of(z)
    ref, bd = epilogue(beta, 0.0, s, ds, np.float64(kap), 0.0)
    return ref, bd, hid, z


def row_ceiling(ref, bd, keep=None):
    """the largest bound of each row over the row's largest |reference| (rows left out, and rows that are exactly 0 with a 0 bound, excluded)"""
    top = np.abs(ref).max(-1)
    b = bd.max(-1)
    ok = (top > 0) | (b > 0)
    if keep is not None:
        ok &= keep
    return (b[ok] / np.maximum(top[ok], 1e-300)).max()


def compare(label, got, ref, bd, keep=None, alts=None):
    """print the measured maximum beside its bound and assert: finite, within the bound -> the largest share of a bound used.  keep:
    the rows [n,64] compared with ref; alts (form_d): rows compared with the nearest of their variants"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got - ref)
    if keep is not None:
        err = np.where(keep[..., None], err, 0.0)
    share = np.where(bd > 0, err / np.where(bd > 0, bd, 1), np.where(err > 0, np.inf, 0.0))
    k = np.unravel_index(np.argmax(err), err.shape)
    left, top = "", float(share.max())
    w = (np.unravel_index(np.argmax(share), share.shape), "")
    if keep is not None:
        n_alt = 0
        if alts is not None and len(alts[0]):
            ai, ap, rv, bv = alts
            ev = np.abs(got[ai, ap][:, None, :] - rv)
            sv = np.where(bv > 0, ev / np.where(bv > 0, bv, 1), np.where(ev > 0, np.inf, 0.0)).max(-1).min(-1)
            n_alt = len(ai)
            if sv.max() > top:
                top, w = float(sv.max()), ((int(ai[np.argmax(sv)]), int(ap[np.argmax(sv)])), " (no rounding variant fits)")
        left = f"; rows on a tie: {n_alt / keep.size:.2%} held to a variant, {1 - (keep.sum() + n_alt) / keep.size:.2%} left out"
    print(f"{label}: max |device - closed form| {err[k]:.3e} (bound there {bd[k]:.3e}; largest share of a bound {top:.3f}{left})")
    assert np.isfinite(got).all(), label
    assert top <= 1.0, (label, "worst (position, pixel, channel)" + w[1], w[0])
    return top


# ------------------------------------------------------------------ the probe nets of the forms (shared by the CPU and the GPU tests)
SEED = 29


def chunks(n, size=256):
    return [slice(i, min(i + size, n)) for i in range(0, n, size)]


def stem_positions():
    """(a): every pixel for PLANES8 (planes 0 and 111 among them), PIX6 for all 112 planes"""
    return impulse_set(PLANES8, range(112))


def conv_positions(C, off):
    """(c), (d): the impulses (trunk channel, pixel) sent through the stem map ci -> ci + off: PIX6 for every channel that no earlier
    map reaches, every pixel for the channels of chan8 among them"""
    seen = {c for o in sigmas(C) if o < off for c in range(o, o + 112)}
    own = [c for c in range(off, off + 112) if c not in seen]
    return impulse_set([c for c in chan8(C) if c in own], own)


def net_a(C, prec, nb=1):
    return natural(nb, C, SEED, prec)


def net_b(C, prec, nb=1):
    sd = natural(nb, C, SEED + 1, prec)
    stem_grid(sd, C, SEED + 1)
    return sd


def dense_boards(golden_boards):
    """(b): golden positions, an all-ones board and an all-zero board"""
    g = np.asarray(golden_boards, np.int8).reshape(-1, 8, 8, 112)
    return np.concatenate([g, np.ones((1, 8, 8, 112), np.int8), np.zeros((1, 8, 8, 112), np.int8)])


def net_c(C, prec, off, nb=1, blk=0):
    """-> (sd, v0, v1): pass-through stem and conv1, natural conv2 and LN2, transparent SE in block blk; with nb > 1 the other blocks
    are transparent, each with its own natural weights"""
    sd = natural(nb, C, SEED + 2 + blk, prec)
    v0 = passthrough_stem(sd, C, off)
    v1 = passthrough_conv1(sd, C, blk, v0)
    transparent_se(sd, C, blk)
    for b in range(nb):
        if b != blk:
            transparent_block(sd, C, b)
    return sd, v0, v1


def net_d(C, prec, off, nb=1, blk=0):
    """-> (sd, v0): pass-through stem, natural conv1 and LN1, identity conv2, natural LN2, transparent SE"""
    sd = natural(nb, C, SEED + 6 + blk, prec)
    v0 = passthrough_stem(sd, C, off)
    p = f"res_blocks.{blk}."
    sd[p + "conv2.weight"], sd[p + "conv2.bias"] = identity_conv(C), np.zeros(C, np.float32)
    transparent_se(sd, C, blk)
    for b in range(nb):
        if b != blk:
            transparent_block(sd, C, b)
    return sd, v0


def net_e2(C, prec):
    """-> (sd, kap, kap1)"""
    sd = natural(1, C, SEED + 10, prec)
    kap, kap1 = kappa(C, 41), kappa(C, 42)
    constant_layer(sd, "conv_block.1", kap)
    constant_layer(sd, "res_blocks.0.bn1", kap1)
    conv_grid(sd, C, "res_blocks.0.conv2", 43)
    transparent_se(sd, C, 0)
    return sd, kap, kap1


def net_e1(C, prec):
    """-> (sd, kap)"""
    sd = natural(1, C, SEED + 11, prec)
    kap = kappa(C, 44)
    constant_layer(sd, "conv_block.1", kap)
    conv_grid(sd, C, "res_blocks.0.conv1", 45)
    sd["res_blocks.0.conv2.weight"], sd["res_blocks.0.conv2.bias"] = identity_conv(C), np.zeros(C, np.float32)
    transparent_se(sd, C, 0)
    return sd, kap


def net_f(C, prec, bname):
    """-> (sd, kap, beta)"""
    sd = natural(1, C, SEED + 12, prec)
    kap, beta = kappa(C, 46), betas(C)[bname]
    constant_layer(sd, "conv_block.1", kap)
    se_probe(sd, C, 0, beta, 47)
    return sd, kap, beta
