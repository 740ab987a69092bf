"""The yardstick of the rounding tests: probe nets that put a chosen float32 value, exact and NOT representable in the operand format, in
front of every place where the network converts an fp32 activation into a matrix operand, and the closed forms of tests/tower_ref.py,
tests/heads_ref.py and tests/tail_ref.py evaluated at the converted operand.  Plain numpy float64; it imports nothing from the engine or
the oracle (the CPU checks at the end are handed the oracle module).

The other probe nets keep every amplitude far from a rounding tie, so they cannot tell how the device rounds.  These sit ON the decision
points.  THE RULE (tower_ref.r_act, tools/scw.py: e4m3_round, oracle/nn.c): round to nearest, ties to the even code; e4m3 keeps its
subnormals (quantum 2^-9); in fp8 the clamp to +-448 comes first, because the convert that follows overflows to NaN (464 -> 448,
480 -> NaN without it).  `convert` restates the rule by brute force over the table of all finite codes, and the wrong rules a changed
site could follow: truncation, ties away from zero, subnormals flushed, a clamp at 240, no clamp.

THE SITES (csrc/nn_tower32.hpp), the instruction sequence each one runs, and the probe net in front of it:
  1 stem LayerNorm + ReLU -> image of conv1       fmaxf, store_image32 = store4<P, false>   stem a constant layer k0, identity conv1
  2 LN1 + ReLU -> image of conv2                  ln_apply_relu_store = store4<P, true>     LN1 a constant layer k1, identity conv2
  3 block output relu(acc s + res) -> image       fmaxf, store_image32 = store4<P, false>   block 1 gives relu(m / 2 + k0) = x exactly
  4 policy LayerNorm, no ReLU -> image of conv2   store_image32<P, 2> = store4<P, false>    policy LN a constant layer, signed
  5 value LayerNorm + ReLU -> bf16 feature row    fmaxf, pk_bf16 (bf16 at both precisions)  value LN a constant layer, FC1 rows select
  6 SE pool and SE hidden vector -> bf16          f2bf (bf16 at both precisions)            LN2 a constant layer / fc1 bias the value
A constant layer (LayerNorm gain 0, bias k[c]) emits k[c] at every pixel for every input, exactly; per-channel parameters are fp32 on
the device (csrc/weights.hpp), so k[c] may be any float32 (`FREE` names the LayerNorm and SE biases that `representable` must let
pass).  An identity conv (weight 1 on the centre tap) turns the converted operand into the conv output as one exact product.

WHAT CARRIES THE OPERAND TO AN OUTPUT.  Sites 1-3 end in the residual stream (Engine.debug), site 4 in the 4672 log-probabilities,
site 5 in the value.  Behind site 2 lie LN2 and the block epilogue (tower_ref.form_e2 with the operand in place of kap1).  Behind sites
1 and 3 lies conv1's dense LN1 row, which rounds once more at site 2: tower_ref.round_rows / MAX_FLIPS variants as in form (e)-conv1.
So that this second rounding cannot swallow a wrong neighbour, LN1's bias is tuned per channel: y1[c] = DELTA times the change of y1[c]
that one operand step of channel c causes, so a wrong neighbour moves y1[c] by a third of itself in e4m3 (two steps at least) and by
1/32 in bf16 (four steps; a smaller y1 would put a tenth of the row within its own LN1 bound of a tie).  LN2's bias is lifted by LIFT so
that no output of a probe net is cut by the last ReLU.  Values of one net lie within a factor 4 of each other (`probe_sets`): a wrong
neighbour is not hidden by the row's largest element.  At sites 1-3 they fill half of the channels and the other half is 0: a row of
one binade alone has a mean five times its spread, and the one-pass variance of LayerNorm loses that factor squared.

THE SE POOL is the only sum in front of a conversion: 64 equal values, added by halving (in-lane pair, five butterfly levels: every
addition doubles, exact) and scaled by 1/64: the pool is the value itself on the device.  The oracle adds the 64 values one by one in
float32, which is not exact for a 24-bit value: `pool_seq` restates that sum, and the CPU tests hand it to the form.

BOUNDS.  None is new: tower_ref.ln / epilogue / scale_of, heads_ref.K_LN_S73, tail_ref.logp_bound_z / value_bound."""
import functools

import numpy as np

import heads_ref as hr
import scw
import tail_ref as tr
import tower_ref as tw

LIFT = 8.0                 # added to LN2's bias: 0.5 LN2 + res stays positive
DELTA = {"bf16": 32.0, "fp8": 3.0}   # LN1 output of a channel over the change one operand step of that channel causes
SEED = 83
BF16_BINADES = (-7, 0, 9)  # [2^-7, 2^-6) below the e4m3 normals, [1, 2), [2^9, 2^10) above the e4m3 maximum
BIG = np.asarray([448, 432, 464, np.nextafter(np.float32(464), np.float32(np.inf)), 480, 1e4, 3e38], np.float32)   # all become 448
RULES = {"bf16": ("trunc", "away"), "fp8": ("trunc", "away", "flush", "clamp240", "noclamp")}
N_POLICY, N_VALUE = 73, 32
B2 = 0.25                  # site 5: FC2's bias; the balanced sum stays within 0.25 of it, so the value is no tiny number
SITES = ("1", "2", "3", "4", "5", "6p", "6h")
FREE = ("conv_block.1.bias", "bn1.bias", "bn2.bias", "policy_head.model.1.bias", "value_head.conv.1.bias", "se.fc1.bias")


def free_names(sd):
    """the per-channel fp32 parameters of a probe net that carry probe values: any float32"""
    return tuple(n for n in sd if n.endswith(FREE))


# ------------------------------------------------------------------ the rule, by brute force
@functools.lru_cache(None)
def codes(fmt):
    """every finite non-negative value of the format in ascending order (float64); the index is the code"""
    if fmt == "fp8":
        return scw.e4m3_decode(np.arange(0x7f, dtype=np.uint8)).astype(np.float64)
    return (np.arange(0x7f80, dtype=np.uint32) << 16).view(np.float32).astype(np.float64)


def convert(x, fmt, rule="rne"):
    """float32 -> operand value (float64): clamp first (fp8), then the nearest finite code, ties to the even code; or a wrong rule:
    trunc (towards zero), away (ties away from zero), flush (results below 2^-6 become 0), clamp240, noclamp (beyond 464: NaN)"""
    x32 = np.asarray(x, np.float32)
    a = np.abs(x32).astype(np.float64)
    t = codes(fmt)
    nan = np.zeros(a.shape, bool)
    if fmt == "fp8":
        nan = (a > 464.0) & (rule == "noclamp")
        a = np.minimum(a, 240.0 if rule == "clamp240" else 448.0)
    assert (a <= t[-1]).all()
    lo = np.searchsorted(t, a, side="right") - 1
    hi = np.minimum(lo + 1, len(t) - 1)
    dl, dh = a - t[lo], t[hi] - a
    up = (dh < dl) | ((dh == dl) & ((lo % 2 == 1) | (rule == "away")))
    if rule == "trunc":
        up = np.zeros(a.shape, bool)
    r = t[np.where(up & (hi != lo), hi, lo)]
    if rule == "flush":
        r = np.where(r < 2.0 ** -6, 0.0, r)
    return np.where(nan, np.nan, np.copysign(r, x32))


def conv_in(x, fmt, rule=None, relu=False):
    """what a conversion site makes of the float32 value x: the stated rule (tower_ref.r_act) or a wrong one"""
    x = np.asarray(x, np.float32)
    if relu:
        x = np.maximum(x, np.float32(0))
    return tw.r_act(x, fmt) if rule is None else convert(x, fmt, rule)


def spacing(a, fmt):
    """distance from the operand value a to the next code above it (for 0: the smallest such distance of the row)"""
    a = np.abs(np.asarray(a, np.float64))
    _, ex = np.frexp(np.where(a > 0, a, 1.0))
    s = np.ldexp(1.0, ex - 1 - 7) if fmt == "bf16" else np.where(a >= 2.0 ** -6, np.ldexp(1.0, ex - 1 - 3), 2.0 ** -9)
    return np.where(a > 0, s, s[a > 0].min() if (a > 0).any() else 2.0 ** -9)


# ------------------------------------------------------------------ decision points
def midpoints(fmt, e=None):
    """fp8: all 126 midpoints between adjacent finite magnitudes; bf16: the 128 of binade [2^e, 2^(e+1)), the carry among them"""
    if fmt == "fp8":
        t = codes(fmt)
        return (t[:-1] + t[1:]) / 2
    return 2.0 ** e * (1 + (np.arange(128) + 0.5) / 128)


def triples(mid):
    """each midpoint with its two float32 neighbours -> (values float32 [3n], their midpoints [3n])"""
    m = np.asarray(mid, np.float32)
    assert np.array_equal(m.astype(np.float64), mid)
    v = np.stack([np.nextafter(m, np.float32(0)), m, np.nextafter(m, np.float32(np.inf))], 1).ravel()
    return v, np.repeat(np.asarray(mid, np.float64), 3)


def groups(fmt):
    """the decision points in groups within a factor 4: fp8 cut greedily from the smallest midpoint up (10 groups), the values
    that the clamp decides (BIG) in the last; bf16 one group a binade -> [(values, midpoints; NaN where a value has none)]"""
    if fmt == "bf16":
        return [triples(midpoints(fmt, e)) for e in BF16_BINADES]
    mid, out, start = midpoints(fmt), [], 0
    for i in range(1, len(mid) + 1):
        if i == len(mid) or mid[i] > 4 * mid[start]:
            out.append(triples(mid[start:i]))
            start = i
    v, m = out[-1]
    out[-1] = (np.concatenate([v, BIG]), np.concatenate([m, np.full(len(BIG), np.nan)]))
    return out


def probe_sets(fmt, n, signed=False):
    """-> [(v float32 [n], mid float64 [n])]: the values of one probe net each, in shuffled order; mid: the midpoint that a decision
    point belongs to, NaN for the others (the clamp's values, zeros, negatives in front of a ReLU, repeats that fill the net).
    A group larger than n is split.  unsigned (a ReLU follows): 0, -0 and three negatives of the group ride along.  signed (site 4):
    fp8 takes every value with both signs; bf16 gives every other pair of midpoints the negative sign (both parities of the lower
    neighbour meet both signs); 0 and -0 ride along"""
    out = []
    for gi, (v, m) in enumerate(groups(fmt)):
        if signed and fmt == "fp8":
            v, m = np.stack([v, -v], 1).ravel(), np.repeat(m, 2)
        elif signed:
            v = v * np.where((np.arange(len(v)) // 6) % 2 == 1, -1, 1).astype(np.float32)
        sp = [0.0, -0.0] if signed else [0.0, -0.0, -v[1], -v[len(v) // 2], -v[-1]]
        v, m = np.concatenate([np.asarray(sp, np.float32), v]), np.concatenate([np.full(len(sp), np.nan), m])
        k = -(-len(v) // n)
        for ci, (cv, cm) in enumerate(zip(np.array_split(v, k), np.array_split(m, k))):
            fill = np.arange(n - len(cv)) % len(cv)
            cv, cm = np.concatenate([cv, cv[fill]]), np.concatenate([cm, np.full(len(fill), np.nan)])
            p = np.random.default_rng(SEED + 100 * gi + ci).permutation(n)
            out.append((cv[p].astype(np.float32), cm[p]))
    return out


def other_neighbour(v, mid, fmt):
    """the neighbour of the midpoint that the rule does NOT pick for v (NaN where v is no decision point)"""
    t = codes(fmt)
    ok = ~np.isnan(mid)
    lo = t[np.searchsorted(t, np.where(ok, mid, 1.0), side="right") - 1]
    hi = t[np.minimum(np.searchsorted(t, np.where(ok, mid, 1.0), side="right"), len(t) - 1)]
    r = np.abs(tw.r_act(v, fmt))
    assert ((r == lo) | (r == hi) | ~ok).all()
    return np.where(ok, np.copysign(lo + hi - r, v), np.nan)


# ------------------------------------------------------------------ building blocks
@functools.lru_cache(None)
def base(nb, C, prec):
    """the natural weights that every probe net of this shape starts from: the same arrays in every net (read only), so a caller
    checks them once (Case.skip names them)"""
    return tw.natural(nb, C, SEED + nb, prec)


def _identity(sd, name, C):
    sd[name + ".weight"], sd[name + ".bias"] = tw.identity_conv(C), np.zeros(C, np.float32)


def _lift(sd, name):
    sd[name + ".bias"] = (sd[name + ".bias"] + np.float32(LIFT)).astype(np.float32)


def _pow2_scale(a, top):
    """the power of two that brings the largest |a| into [top / 2, top) (1 for an all-zero a)"""
    m = np.abs(a).max()
    return 1.0 if m == 0 else top / 2.0 ** (np.floor(np.log2(m)) + 1)


def _f64(sd, name):
    return np.asarray(sd[name], np.float64)


# ------------------------------------------------------------------ site 2
def net_s2(C, prec, k1):
    """one block: stem a constant layer kap, LN1 the constant layer k1, conv2 the identity, LN2 natural (lifted), SE transparent"""
    sd, p = dict(base(1, C, prec)), "res_blocks.0."
    kap = tw.kappa(C, 41)
    tw.constant_layer(sd, "conv_block.1", kap)
    tw.constant_layer(sd, p + "bn1", k1)
    _identity(sd, p + "conv2", C)
    _lift(sd, p + "bn2")
    tw.transparent_se(sd, C, 0)
    return sd, kap


def rows_s2(sd, kap, A):
    """stage 1 for conv2 operand rows A[V,C] (every pixel the same): relu(0.5 LN2(A) + kap) -> (ref [V,C], bound)"""
    y, d = tw.ln(A, _f64(sd, "res_blocks.0.bn2.weight"), _f64(sd, "res_blocks.0.bn2.bias"))
    return tw.epilogue(y, d, tw.HALF[0], tw.HALF[1], np.float64(kap)[None, :], 0.0)


def form_s2(sd, prec, kap, k1, rule=None):
    """tower_ref.form_e2's chain with the converted k1 in place of kap1 -> (stage 1 [64][C], bound)"""
    return tw.form_e2(sd, 0, kap, conv_in(k1, prec, rule, True))


# ------------------------------------------------------------------ sites 1 and 3: a block behind the probed value
def _probe_block(sd, C, prec, blk, x_in, quiet):
    """in place: block blk behind the residual stream x_in[c] >= 0 (the same at every pixel): identity conv1, LN1 with its natural
    gain and the tuned bias (module docstring; negative in the channels `quiet`, the half that carries no probe value: LN2's row is
    then half zeros, and as well conditioned as LN1's), identity conv2, LN2 natural (lifted), SE transparent"""
    p = f"res_blocks.{blk}."
    _identity(sd, p + "conv1", C)
    _identity(sd, p + "conv2", C)
    _lift(sd, p + "bn2")
    tw.transparent_se(sd, C, blk)
    a, g1 = tw.r_act(x_in, prec), _f64(sd, p + "bn1.weight")
    sig = np.sqrt(a.var() + tw.EPS)
    assert (g1 > 0).all()
    sd[p + "bn1.bias"] = (np.where(quiet, -1, 1) * DELTA[prec] * g1 * spacing(a, prec) / sig - g1 * (a - a.mean()) / sig).astype(np.float32)


def rows_block(sd, prec, blk, A, x_in):
    """stage blk+1 for conv1 operand rows A[V,C] behind the residual x_in[C] -> (ref [V,C], bound, and round_rows' four results)"""
    p = f"res_blocks.{blk}."
    y1, d1 = tw.ln(A, _f64(sd, p + "bn1.weight"), _f64(sd, p + "bn1.bias"))
    base, dx2, flip, alt = tw.round_rows(y1, d1, prec)
    y2, d2 = tw.ln(base, _f64(sd, p + "bn2.weight"), _f64(sd, p + "bn2.bias"), dx2)
    ref, bd = tw.epilogue(y2, d2, tw.HALF[0], tw.HALF[1], np.float64(x_in)[None, :], 0.0)
    return ref, bd, base, dx2, flip, alt


def form_block(sd, prec, blk, x_in, rule=None):
    """-> (stage blk+1 [1][1][C], bound, keep [1][1], alts) as tower_ref.form_e1: the one row that every pixel shows"""
    p = f"res_blocks.{blk}."
    ref, bd, base, dx2, flip, alt = rows_block(sd, prec, blk, conv_in(x_in, prec, rule)[None, :], x_in)
    nf = flip.sum(-1)
    ap = np.flatnonzero((nf > 0) & (nf <= tw.MAX_FLIPS))
    yv, dv = tw._variants(base[ap], dx2[ap], flip[ap], alt[ap], _f64(sd, p + "bn2.weight"), _f64(sd, p + "bn2.bias"))
    rv, bv = tw.epilogue(yv, dv, tw.HALF[0], tw.HALF[1], np.float64(x_in)[None, None, :], 0.0)
    return ref[None], bd[None], (nf == 0)[None], (np.zeros(len(ap), np.int64), ap, rv, bv)


def net_s1(C, prec, k0, quiet):
    """one block behind the stem as the constant layer k0 -> (sd, the residual stream relu(k0))"""
    sd = dict(base(1, C, prec))
    tw.constant_layer(sd, "conv_block.1", k0)
    x = np.maximum(np.asarray(k0, np.float32), np.float32(0))
    _probe_block(sd, C, prec, 0, x, quiet)
    return sd, x


def split_s3(x):
    """-> (k0 >= 0, m) with relu(m * 0.5 + k0) = relu(x) exactly in float32: k0 the upper 8 bits of a positive x, m twice the rest;
    from 1024 on k0 = x and m = 0, and m stops at -1024 (the SE pool in between adds 64 values m: it must stay finite)"""
    x = np.asarray(x, np.float32)
    small = np.abs(x) < 1024
    hi = np.where((x > 0) & small, (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32), np.where(x > 0, x, np.float32(0)))
    m = np.where(x > 0, (np.where(small, x, 0) - np.where(small, hi, 0)) * np.float32(2), np.maximum(x, np.float32(-1024))).astype(np.float32)
    assert np.array_equal(np.maximum(m * np.float32(0.5) + hi, np.float32(0)), np.maximum(x, np.float32(0)))
    assert np.array_equal(np.float64(m) * 0.5 + np.float64(hi), np.where(x > 0, np.float64(x), np.float64(m) * 0.5))   # no rounding at all
    return hi.astype(np.float32), m


def net_s3(C, prec, x, quiet):
    """two blocks: block 1 has LN2 the constant layer m and a transparent SE over the constant stem k0, so stage 1 is relu(x); block
    2 is the probe block -> (sd, relu(x))"""
    sd = dict(base(2, C, prec))
    k0, m = split_s3(x)
    tw.constant_layer(sd, "conv_block.1", k0)
    tw.constant_layer(sd, "res_blocks.0.bn2", m)
    tw.transparent_se(sd, C, 0)
    xr = np.maximum(np.asarray(x, np.float32), np.float32(0))
    _probe_block(sd, C, prec, 1, xr, quiet)
    return sd, xr


# ------------------------------------------------------------------ site 4
def _chan(n, idx):
    return np.random.default_rng(SEED + 7 * idx).permutation(hr.HEAD)[:n]


def net_s4(C, prec, v, idx):
    """no block: policy LayerNorm the constant layer k (v at 73 of its 256 channels), policy conv2 reads one of them per output
    plane through one power-of-two weight, the 73-wide LayerNorm natural -> (sd, channels, weight)"""
    sd = dict(base(0, C, prec))
    ch = _chan(N_POLICY, idx)
    k = np.zeros(hr.HEAD, np.float32)
    k[ch] = v
    tw.constant_layer(sd, "policy_head.model.1", k)
    w = _pow2_scale(tw.r_act(v, prec), 4.0)
    W = np.zeros((N_POLICY, hr.HEAD, 1, 1), np.float32)
    W[np.arange(N_POLICY), ch, 0, 0] = w
    sd["policy_head.model.2.weight"], sd["policy_head.model.2.bias"] = W, np.zeros(N_POLICY, np.float32)
    return sd, ch, w


def rows_s4(sd, w, A):
    """log-probabilities for conv2 operand rows A[V,73] (every pixel the same) -> (logp [V,4672], bound): conv2's output w A is one
    exact product, then heads_ref's 73-wide LayerNorm and tail_ref's log-softmax, action = plane * 64 + pixel"""
    y, dy = tw.ln(w * np.asarray(A, np.float64), _f64(sd, "policy_head.model.3.weight"), _f64(sd, "policy_head.model.3.bias"),
                  k_s=hr.K_LN_S73, k_inv=1)
    y, dy = np.repeat(y, 64, axis=-1), np.repeat(dy, 64, axis=-1)
    if np.isnan(y).any():
        return y, dy
    return np.stack([tr.logp_closed_z(r) for r in y]), np.stack([tr.logp_bound_z(r, d) for r, d in zip(y, dy)])


def form_s4(sd, prec, w, v, rule=None):
    lp, bd = rows_s4(sd, w, conv_in(v, prec, rule)[None, :])
    return lp[0], bd[0]


# ------------------------------------------------------------------ site 5
def net_s5(C, prec, v, idx):
    """no block: value LayerNorm the constant layer k (v at 32 of its 256 channels); FC1 row j reads feature (channel j, pixel j)
    through one power-of-two weight, no meta columns, no bias; FC2 weights +-1/32 with signs that balance the sum (the tanh argument
    stays near the bias B2, inside (-2.8, 2.8)) -> (sd, w, w2)"""
    sd = dict(base(0, C, prec))
    ch, px = _chan(N_VALUE, idx), (7 * np.arange(N_VALUE) + 3) % 64
    k = np.zeros(hr.HEAD, np.float32)
    k[ch] = v
    tw.constant_layer(sd, "value_head.conv.1", k)
    a = tw.r_act(np.maximum(v, 0), "bf16")
    w = _pow2_scale(a, 2.0)
    W1 = np.zeros((128, 64 * hr.HEAD + 7), np.float32)
    W1[np.arange(N_VALUE), ch * 64 + px] = w
    w2, run = np.zeros(128), 0.0
    for j in np.argsort(-a, kind="stable"):
        w2[j] = -1 / 32.0 if run > 0 else 1 / 32.0
        run += w2[j] * a[j] * w
    assert abs(run) < 0.25
    sd["value_head.ffn.0.weight"], sd["value_head.ffn.0.bias"] = W1, np.zeros(128, np.float32)
    sd["value_head.ffn.2.weight"], sd["value_head.ffn.2.bias"] = w2.astype(np.float32).reshape(1, 128), np.full(1, B2, np.float32)
    return sd, w, w2


def rows_s5(w, w2, A, meta, k_fc2=tr.K_FC2_DEVICE):
    """values for feature rows A[n,32] (bf16 values) and meta[n,7] -> (value [n], bound): FC1's output w A is one exact product a
    unit, the rest is tail_ref's value tail"""
    h = np.zeros((len(A), 128))
    h[:, :N_VALUE] = w * np.asarray(A, np.float64)
    p = (np.zeros((128, 7)), np.zeros(128), w2, B2)
    assert (np.abs(tr.value_args(meta, *p, feat=np.nan_to_num(h))) < 2.8).all()
    return tr.value_closed(meta, *p, feat=h), tr.value_bound(meta, *p, k_fc2=k_fc2, feat=h)


def form_s5(w, w2, v, meta, rule=None, k_fc2=tr.K_FC2_DEVICE):
    return rows_s5(w, w2, np.broadcast_to(conv_in(v, "bf16", rule, True), (len(meta), N_VALUE)), meta, k_fc2)


# ------------------------------------------------------------------ site 6
def net_s6(C, prec, v, idx, what):
    """one block over a zero stem, LN2 a constant layer m, so that stage 1 is relu(m sigma(z)).  what = "p", the pool: v sits in m at
    C/2 channels `src` (1 elsewhere), fc1 unit j reads pool channel src[j] through one power-of-two weight, fc2 shows unit j at
    channel dst[j].  what = "h", the hidden vector: m = 1, fc1 has no weights and the bias v, fc2 shows unit j at src[j] and, negated,
    at dst[j] -> (sd, m)"""
    sd, p, H = dict(base(1, C, prec)), "res_blocks.0.", C // 2
    tw.constant_layer(sd, "conv_block.1", np.zeros(C, np.float32))
    perm = np.random.default_rng(SEED + 11 * idx).permutation(C)
    src, dst, j = perm[:H], perm[H:], np.arange(H)
    m, W1, W2, b1 = np.ones(C, np.float32), np.zeros((H, C), np.float32), np.zeros((C, H), np.float32), np.zeros(H, np.float32)
    w = _pow2_scale(tw.r_act(np.maximum(v, 0), "bf16"), 2.0)
    if what == "p":
        m[src], W1[j, src], W2[dst, j] = v, w, 1.0
    else:
        b1, W2[src, j], W2[dst, j] = np.asarray(v, np.float32), w, -w
    tw.constant_layer(sd, p + "bn2", m)
    sd[p + "se.fc1.weight"], sd[p + "se.fc1.bias"] = W1.reshape(H, C, 1, 1), b1
    sd[p + "se.fc2.weight"], sd[p + "se.fc2.bias"] = W2.reshape(C, H, 1, 1), np.zeros(C, np.float32)
    return sd, m


def pool_seq(m):
    """the oracle's pool of 64 equal values m[c]: added one by one in float32, divided by 64"""
    s = np.zeros(len(m), np.float32)
    for _ in range(64):
        s = s + np.asarray(m, np.float32)
    return s / np.float32(64)


def form_s6(sd, m, rule_pool=None, rule_hidden=None, pool=None, other=None):
    """stage 1 [C] = relu(m sigma(fc2(bf16(relu(fc1(bf16(pool)) + b1))))) -> (ref, bound): every fc sum is one exact product or the
    bias alone; pool: what the average of 64 values m came to (m itself on the device); other = (unit, value): that hidden unit's
    operand replaced"""
    p, C = "res_blocks.0.se.", len(m)
    W1, W2 = _f64(sd, p + "fc1.weight").reshape(C // 2, C), _f64(sd, p + "fc2.weight").reshape(C, C // 2)
    assert ((W1 != 0).sum(1) <= 1).all() and ((W2 != 0).sum(1) <= 1).all() and not (W1.any() and sd[p + "fc1.bias"].any())
    pl = conv_in(m if pool is None else pool, "bf16", rule_pool)
    t = (W1 * pl[None, :]).sum(1) + _f64(sd, p + "fc1.bias")
    assert np.array_equal(np.nan_to_num(t), np.nan_to_num(np.float32(t).astype(np.float64)))
    hid = conv_in(t, "bf16", rule_hidden, True)
    if other is not None:
        hid = hid.copy()
        hid[other[0]] = other[1]
    s, ds = tw.scale_of((W2 * hid[None, :]).sum(1) + _f64(sd, p + "fc2.bias"))
    return tw.epilogue(np.float64(m), 0.0, s, ds, 0.0, 0.0)


# ------------------------------------------------------------------ the probe nets of a site, one interface for the CPU and the GPU tests
class Case:
    """one probe net: sd, nb blocks; the output it is read from (`kind`: "stage" = the residual stream after the last block, "logp",
    "value"); v / mid: its probe values and their midpoints (probe_sets); fmt: the operand format of the site"""

    def __init__(self, site, C, prec, idx, v, mid):
        self.site, self.C, self.prec, self.idx, self.v, self.mid = site, C, prec, idx, v, mid
        self.fmt = "bf16" if site in ("5", "6p", "6h") else prec
        self.kind = {"4": "logp", "5": "value"}.get(site, "stage")
        self.nb = {"3": 2, "4": 0, "5": 0}.get(site, 1)
        self.meta = hr.metas(7)
        if site in ("1", "2", "3"):        # the other half of the channels: 0
            p = np.random.default_rng(SEED + 13 * idx).permutation(C)
            v, mid = np.concatenate([v, np.zeros(C // 2, np.float32)])[p], np.concatenate([mid, np.full(C // 2, np.nan)])[p]
            self.v, self.mid, quiet = v, mid, p >= C // 2
        if site == "1":
            self.sd, self.x = net_s1(C, prec, v, quiet)
        elif site == "2":
            self.sd, self.kap = net_s2(C, prec, v)
        elif site == "3":
            self.sd, self.x = net_s3(C, prec, v, quiet)
        elif site == "4":
            self.sd, self.ch, self.w = net_s4(C, prec, v, idx)
        elif site == "5":
            self.sd, self.w, self.w2 = net_s5(C, prec, v, idx)
        else:
            self.sd, self.m = net_s6(C, prec, v, idx, site[1])
        self.skip = free_names(self.sd) + tuple(n for n, a in self.sd.items() if a is base(self.nb, C, prec).get(n))

    def label(self):
        return f"{self.C} {self.prec} site {self.site} net {self.idx}"

    def form(self, rule=None, oracle=False):
        """-> the arguments of tower_ref.compare behind `got`: stage [1][1][C] (every pixel of every position is this row), logp
        [4672], value [7] for `meta`.  oracle: the oracle's order of the pool sum and of FC2"""
        s = self.site
        if s == "2":
            ref, bd = form_s2(self.sd, self.prec, self.kap, self.v, rule)
            assert all(np.array_equal(ref[0], r, equal_nan=True) for r in ref)
            return ref[None, :1], bd[None, :1]
        if s in ("1", "3"):
            return form_block(self.sd, self.prec, self.nb - 1, self.x, rule)
        if s == "4":
            return form_s4(self.sd, self.prec, self.w, self.v, rule)
        if s == "5":
            return form_s5(self.w, self.w2, self.v, self.meta, rule, tr.K_FC2_ORACLE if oracle else tr.K_FC2_DEVICE)
        ref, bd = form_s6(self.sd, self.m, rule if s == "6p" else None, rule if s == "6h" else None, pool_seq(self.m) if oracle else None)
        return ref[None, None], bd[None, None]

    def others(self):
        """for every decision point of the net: how far the output element that shows it moves when the OTHER neighbour of its
        midpoint is the operand, over the bound there -> ratios [points]"""
        i = np.flatnonzero(~np.isnan(self.mid))
        if not len(i):
            return np.zeros(0)
        relu = self.site != "4"
        a = conv_in(self.v, self.fmt, None, relu)
        o = other_neighbour(self.v, self.mid, self.fmt)[i]
        s = self.site
        if s in ("1", "2", "3", "4", "5"):
            A = np.repeat(a[None, :], len(i), 0)
            A[np.arange(len(i)), i] = o
        if s == "2":
            (r0, b0), (r1, _) = rows_s2(self.sd, self.kap, a[None]), rows_s2(self.sd, self.kap, A)
            return np.abs(r1[np.arange(len(i)), i] - r0[0, i]) / b0[0, i]
        if s in ("1", "3"):
            r0, b0 = rows_block(self.sd, self.prec, self.nb - 1, a[None], self.x)[:2]
            r1 = rows_block(self.sd, self.prec, self.nb - 1, A, self.x)[0]
            return np.abs(r1[np.arange(len(i)), i] - r0[0, i]) / b0[0, i]
        if s == "4":
            (r0, b0), (r1, _) = rows_s4(self.sd, self.w, a[None]), rows_s4(self.sd, self.w, A)
            return np.abs(r1[np.arange(len(i)), i * 64] - r0[0, i * 64]) / b0[0, i * 64]
        if s == "5":
            (r0, b0), (r1, _) = rows_s5(self.w, self.w2, a[None], self.meta[:1]), rows_s5(self.w, self.w2, A, np.repeat(self.meta[:1], len(i), 0))
            return np.abs(r1 - r0[0]) / b0[0]
        perm = np.random.default_rng(SEED + 11 * self.idx).permutation(self.C)
        show = perm[self.C // 2:] if s == "6p" else perm[:self.C // 2]
        r0, b0 = form_s6(self.sd, self.m)
        scale = np.abs(_f64(self.sd, "res_blocks.0.se.fc2.weight")).max() if s == "6h" else np.abs(_f64(self.sd, "res_blocks.0.se.fc1.weight")).max()
        out = []
        for j, oj in zip(i, o):
            r1, _ = form_s6(self.sd, self.m, other=(j, oj * (scale if s == "6p" else 1.0)))
            out.append(abs(r1[show[j]] - r0[show[j]]) / b0[show[j]])
        return np.asarray(out)


def n_slots(site, C):
    return {"4": N_POLICY, "5": N_VALUE}.get(site, C // 2)


def precisions(site, prec):
    """sites 5 and 6 are bf16 at both precisions"""
    return "bf16" if site in ("5", "6p", "6h") else prec


def cases(site, C, prec):
    """the probe nets of a site, one after the other"""
    for idx, (v, mid) in enumerate(probe_sets(precisions(site, prec), n_slots(site, C), signed=site == "4")):
        yield Case(site, C, prec, idx, v, mid)


class OracleNet:
    """one oracle network (the module `orc` = oracle.oracle_py) for many probe nets of the same shape: only the tensors that
    differ from the last net are set again"""
    MODE = {"bf16": dict(emulate_bf16=True), "fp8": dict(emulate_fp8=True)}

    def __init__(self, orc, nb, C, prec):
        self.net, self.table, self.cur = orc.Net(nb, C, seed=1, **self.MODE[prec]), scw.tensor_table(nb, C), {}

    def run(self, sd, boards, meta):
        """-> (logp [n,4672], value [n], latent [n,64,C])"""
        for i, (name, _, _, _) in enumerate(self.table):
            if self.cur.get(name) is not sd[name]:
                self.net.set_tensor(i, sd[name])
                self.cur[name] = sd[name]
        res = [self.net.forward(b, m, latent=True) for b, m in zip(boards, meta)]
        return np.stack([r[0] for r in res]), np.asarray([r[1] for r in res], np.float32), np.stack([r[2] for r in res])


def oracle_output(cache, orc, c, nb=None):
    """what the oracle makes of case c, as Case.form expects it (stage [1][1][C], logp [4672], value [7]), after checking that every
    pixel and every position agree.  cache: a dict that keeps one OracleNet per shape.  nb: cut the net after nb blocks"""
    nb = c.nb if nb is None else nb
    key = (nb, c.C, c.prec)
    if key not in cache:
        cache[key] = OracleNet(orc, nb, c.C, c.prec)
    b = np.zeros((2, 8, 8, 112), np.int8)
    b[1, ::2, 1::3, ::5] = 1
    if c.kind == "value":
        return cache[key].run(c.sd, b[np.arange(len(c.meta)) % 2], c.meta)[1]
    lp, _, lat = cache[key].run(c.sd, b, c.meta[:2])
    if c.kind == "logp":
        assert np.array_equal(lp[0], lp[1])
        return lp[0]
    assert all(np.array_equal(lat[0, 0], r) for g in lat for r in g)
    return lat[:1, :1]


# ------------------------------------------------------------------ the CPU checks of a site (tests/test_tower_ref.py, tests/test_heads_ref.py)
def check_site(orc, site, C, prec):
    """every probe net of a site: representable, the oracle inside the bounds of the form, every row compared (none left out: each
    net is one row, so every probed channel keeps its row), every bound under the ceiling, and the OTHER neighbour of every decision
    point at least TIE_SAFETY bounds away at the element that shows it"""
    cache, top, ratio, ceil, held, points, nets = {}, 0.0, np.inf, 0.0, 0, 0, 0
    tw.representable(base({"3": 2, "4": 0, "5": 0}.get(site, 1), C, prec), prec)
    for c in cases(site, C, prec):
        tw.representable(c.sd, prec, c.skip)
        assert all(n.endswith(".bias") for n in free_names(c.sd))          # conv weights stay representable
        if site == "3":
            assert np.array_equal(oracle_output(cache, orc, c, nb=1)[0, 0], c.x)
        f = c.form(oracle=True)
        top = max(top, tw.compare("oracle " + c.label(), oracle_output(cache, orc, c), *f))
        if len(f) == 4:
            assert f[2].all() or len(f[3][0]), (c.label(), "the net's one row has more than MAX_FLIPS elements on a tie")
            held += len(f[3][0])
            ceil = max(ceil, tw.row_ceiling(f[3][2], f[3][3]) if len(f[3][0]) else 0.0)
        ceil = max(ceil, float(np.max(f[1]) / np.abs(f[0]).max()))
        r = c.others()
        ratio, points, nets = min([ratio] + list(r)), points + len(r), nets + 1
    print(f"oracle {C} {prec} site {site}: {points} decision points in {nets} nets; largest share of a bound {top:.3f}; the other neighbour "
          f"lies >= {ratio:.0f} bounds away; largest bound / row maximum {ceil:.2e}; rows held to a rounding variant {held}, left out 0")
    assert ratio >= tw.TIE_SAFETY and ceil <= tw.CEIL
    return points


def check_wrong_rules(orc, site, C, prec):
    """forms built from the wrong rules of the site's operand format must each miss the oracle on at least one probe net"""
    cache, todo = {}, None
    for c in cases(site, C, prec):
        todo = set(RULES[c.fmt]) if todo is None else todo
        got = oracle_output(cache, orc, c)
        for rule in sorted(todo):
            with np.errstate(all="ignore"):
                f = c.form(rule, oracle=True)
            if np.isnan(f[0]).any():              # the rule gives NaN where the oracle is finite (compare asserts that)
                assert np.isfinite(got).all()
                todo.discard(rule)
                continue
            try:
                tw.compare(f"{c.label()}, form with rule {rule}", got, *f)
            except AssertionError:
                todo.discard(rule)
    assert not todo, (site, C, prec, "wrong rules that no probe net catches", todo)
