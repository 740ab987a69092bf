"""The yardstick of the LayerNorm offset tests: rows with a large common offset in front of each of the network's six LayerNorms, the
float64 two-pass LayerNorm they are held to, and the envelope -- up to which mean / sigma the engine keeps to that operation.

WHY.  The engine's LayerNorm is one pass (csrc/nn_tower32.hpp: ln_reduce): var = Q / C - mean^2, clamped at 0.  The reference's
(timm LayerNorm2d = F.layer_norm) and the oracle's (oracle/nn.c: layernorm) are two passes.  They differ by about U mean^2 / var in
the variance, so the loss grows with the square of mean / sigma; past the point where the variance clamps to 0 the outputs are finite
and wrong, and nothing in the engine flags them.  tower_ref.ln carries that cancellation in its BOUND, which therefore grows with the
error; every other probe of the suite keeps mean / sigma below a few.  This module is plain numpy float64; it imports nothing from
the engine or the oracle (the measurement of R_REQ at the end is handed the oracle module).

THE ROW.  x[c] = M + s d[c]: d a fixed pattern on the 1/4 grid with an exactly zero sum and a known sum of squares (`pattern`:
+-k/4, k = 1..6, in pairs, one 0 where the width is odd; sigma = 0.96 at 128, 256 and 73 channels), s a power of two, M = +-m s
with m one of RUNGS, so mean / sigma = 1.04 m.  Every x[c] is exact in float32 (asserted).  The rungs run at s = 1; the 64 and 512
rungs again at s = 2^-8 (var 1.4e-5: eps = 1e-6 takes part) and 2^8.  `rows` lists the rows as (m, sign, log2 s[, off the grid]).  Up to m = 64 the sums S and
Q of such a row are themselves exact in float32 (multiples of s/4 and s^2/16 below 2^24 units), so where 1 / width is a power of two
the one-pass variance loses nothing yet and the error is the apply step's; the 73-wide site, whose 1 / 73 is rounded, shows the
growth with the square of the ratio from the first rung on.  So that the rungs up to R_REQ, where assertion 2 binds, meet the
cancellation at every site, the rungs 8, 64 and 512 run once more with d OFF the grid (13 more bits an element, the same exact
zero sum and known sum of squares): 6 more rows, 25 in all.

HOW THE ROW REACHES A LAYERNORM EXACTLY.  The conv in front of it gets zero weights and the row as its bias: conv biases stay fp32 on
the device (csrc/weights.hpp: pack), the accumulator is the bias plus products of zeros, so the LayerNorm's input is x at every pixel
of every position, with no operand rounding in front of it.  Three nets carry the six sites (`Net`):
  net "s" (no block)   stem LN: stem conv = row; natural gain, bias lifted by LIFT: stage 0, nothing cut by the ReLU.
                       policy LN1: policy conv1 = row; natural gain, zero bias, no ReLU; its rounded output is the operand of a grid
                       conv2 (1/8 grid, exact sums), then the natural 73-wide LayerNorm and the log-softmax.
  net "a" (one block)  LN1: constant stem kap, conv1 = row, natural LN1 (ReLU); its rounded output passes the identity conv2, the
                       natural LN2 (lifted) and the transparent SE: stage 1 = relu(0.5 LN2(operand) + kap).
  net "b" (one block)  LN2: constant stem kap, constant LN1, conv2 = row, natural LN2 (lifted), transparent SE: stage 1 =
                       relu(0.5 LN2(row) + kap).  policy LN, 73 wide: policy conv2 = row, natural gain and bias: the 4672
                       log-probabilities y[c] - log(64 sum exp y).  value LN: value conv = row, natural gain, bias lifted; its bf16
                       features (ReLU cuts nothing) go through an FC1 whose unit j adds channels j and j + 128 at one pixel each,
                       and an FC2 of +-1/32 whose signs balance the sum: the value.

THE YARDSTICK is tower_ref.ln's VALUE, the float64 two-pass LayerNorm with eps 1e-6: the operation of the reference.  Its BOUND is the
one-pass fp32 model.  Two assertions use them (tests/test_gpu_ln_offset.py on the device, tests/test_tower_ref.py and
tests/test_heads_ref.py on the oracle and on a deliberately one-pass LayerNorm):
  1  every rung: finite, and |device - exact| within the one-pass bound carried to the observed output (`Site.check1`).  At the three
     sites behind a rounding the device's operand lies between the roundings of exact -+ bound; that interval is the input error of
     the layers behind it.
  2  the operation, `Site.check2`.  At the three fp32 sites |device - exact| <= max(half an operand ulp of |exact|, 2^-9 of the row's
     largest |exact|) -- bf16 ulps at bf16, e4m3 ulps at fp8 -- the error is then invisible next to the operand rounding that follows
     every LayerNorm of this network.  Stem and LN2 take this on the observed stage.  The 73-wide LayerNorm is seen through the
     log-softmax, whose log(4672) would widen an ulp taken on the log-probabilities: the tolerance is taken on the LayerNorm's own
     output y and carried through tail_ref.logp_bound_z (its own share plus the softmax-weighted mean), which is never wider.
     At the three sites behind a rounding the operand the device forms must BE the rounding of the exact LayerNorm: the output
     must match the closed form behind that operand within the bound of the layers behind it alone.  Only elements whose exact value
     lies within assertion 1's bound of a rounding tie may round either way (every combination is tried); at most `cap` of a row's
     elements, 2 % and never more than tower_ref.MAX_FLIPS, may be excused: in a row with more, none is, and the operand must be the
     reference's own rounding throughout.  So that this asks for the operation and not for luck, the LayerNorm bias of these three
     sites puts every exact output ON a code of the operand format (`Net`: the middle of its rounding cell): the operand flips only
     when the error reaches half an ulp, the criterion of the fp32 sites, and up to R_REQ no element of the reference lies within
     the one-pass bound of a tie (`check_conditions`).
Both derive their bounds from the exact values alone.

THE ENVELOPE.  R_REQ is the rung the engine must reach: the next rung at or above 8 times the largest mean / sigma that any
LayerNorm input of the project's own networks shows (`measure_ratios`, float64 statistics of the oracle; DESIGN.md section 7 holds the
table and says why 8).  Up to R_REQ every site must meet 2.  Above it the tests print what they measure, assert 1, and assert that
the first rung that fails 2 is ENVELOPE[site, C, precision]: a change that moves the envelope either way has to move that constant."""
import functools
import itertools

import numpy as np

import scw
import heads_ref as hr
import tail_ref as tr
import tower_ref as tw

U = tr.U
RUNGS = (0, 8, 64, 512, 4096, 32768)
LOG2_S = (-8, 8)           # the 64 and 512 rungs again at these scales
OFF_GRID_RUNGS = (8, 64, 512)          # ... and these rungs again with d off the 1/4 grid (`pattern`); 4096 + d would need 25 bits
LIFT = 4.0                 # stem, LN2, value LayerNorm: added to the natural bias
B2 = 0.25                  # FC2's bias at the value site
SEED = 97
SITES = ("stem", "ln2", "p73", "ln1", "vln", "pln1")
NETS = {"s": ("stem", "pln1"), "a": ("ln1",), "b": ("ln2", "p73", "vln")}
CAP_SHARE = 0.02           # assertion 2 behind a rounding: the share of a row's elements that may sit on a tie

# DESIGN.md section 7, "LayerNorm inputs: mean / sigma of the project's networks": the largest ratio found is 0.36 (the 73-wide
# policy LayerNorm of the 1 x 256 network), 8 times that is 2.9, the next rung is 8
R_REQ = 8
LARGEST_RATIO = 0.357      # the largest entry of RATIOS below (tests/test_tower_ref.py measures the table again)
# (site, C, precision) -> the first rung that fails assertion 2 on the device (None: none does); measured on an MI355X, DESIGN.md
# section 7
_FIRST_FAILING = {"bf16": dict(stem=512, ln2=512, p73=512, ln1=512, vln=512, pln1=512),
                  "fp8": dict(stem=4096, ln2=4096, p73=4096, ln1=4096, vln=512, pln1=4096)}       # the same at 128 and 256 channels
ENVELOPE = {(s, C, p): _FIRST_FAILING[p][s] for s in SITES for C in (128, 256) for p in ("bf16", "fp8")}


# ------------------------------------------------------------------ rows
def pattern(width, off_grid=0):
    """d[width] on the 1/4 grid: pairs +-k/4 with k cycling through 1..6, one 0 where the width is odd, shuffled; sum 0 (asserted),
    -> (d, sum of squares).  off_grid: pair i is +-(k/4 + j_i 2^-12) with odd j_i below 64 instead: still an exact zero sum and an
    exactly known sum of squares, but 13 more bits an element, so the float32 sums S and Q of a row round from the first rung on"""
    k = (1 + np.arange(width // 2) % 6) * 1024
    if off_grid:
        k = k + 2 * np.random.default_rng(SEED + 7 * width).integers(0, 32, width // 2) + 1
    d = np.concatenate([k, -k, np.zeros(width % 2, np.int64)])
    d = d[np.random.default_rng(SEED + width).permutation(width)]
    ss = 2 * int((k * k).sum())
    assert d.sum() == 0 and int((d * d).sum()) == ss and (off_grid or not (d % 1024).any())
    return d / 4096.0, ss / 4096.0 ** 2


def rows():
    """[(m, sign, log2 s[, 1])]: every rung at s = 1 with both signs of M (m = 0 once), the 64 and 512 rungs at the two other
    scales, the rungs of OFF_GRID_RUNGS with d off the grid (the fourth element)"""
    out = [(0, 1, 0)] + [(m, sg, 0) for m in RUNGS[1:] for sg in (1, -1)]
    out += [(m, sg, ls) for ls in LOG2_S for m in (64, 512) for sg in (1, -1)]
    return out + [(m, sg, 0, 1) for m in OFF_GRID_RUNGS for sg in (1, -1)]


def row(width, m, sign, log2s, off_grid=0):
    """x[width] = s (sign m + d), exact in float32 (asserted)"""
    d, ss = pattern(width, off_grid)
    x = np.ldexp(sign * m + d, log2s)
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
    assert x.mean() == np.ldexp(float(sign * m), log2s) and ((x - x.mean()) ** 2).sum() == np.ldexp(ss, 2 * log2s)
    return x


def label(r):
    return f"m {r[1] * r[0]:+d} s 2^{r[2]}" + (" off the grid" if len(r) > 3 else "")


def half_ulp(a, prec):
    """half the spacing of the operand format at |a| (bf16: 8 significant bits; e4m3: 4, quantum 2^-9 below 2^-6)"""
    a = np.abs(np.asarray(a, np.float64))
    _, ex = np.frexp(np.where(a > 0, a, 1.0))
    if prec == "bf16":
        return np.where(a > 0, np.ldexp(1.0, ex - 1 - 8), 0.0)
    return np.where(a >= 2.0 ** -6, np.ldexp(1.0, ex - 1 - 4), 2.0 ** -10)


def operand_tol(exact, prec):
    """assertion 2 at an fp32 site: max(half an operand ulp of |exact|, 2^-9 of the row's largest |exact|)"""
    exact = np.asarray(exact, np.float64)
    return np.maximum(half_ulp(exact, prec), 2.0 ** -9 * np.abs(exact).max(-1, keepdims=True))


def one_pass32(x, g, e):
    """a deliberately WRONG LayerNorm for this module's yardstick: the one-pass formula of ln_reduce / ln_apply restated in numpy
    float32, roughly in its order -- four waves of two lane halves of two packed partial sums each, summed in turn, then pairwise;
    the width padded with zeros to a multiple of 128, 1 / width rounded"""
    f = np.float32
    x32 = np.asarray(x, f)
    n = len(x32)
    pad = np.concatenate([x32, np.zeros(-n % 128, f)]).reshape(4, 2, -1, 2)          # wave, lane half, register pair, packed half
    S, Q = np.zeros((4, 2, 2), f), np.zeros((4, 2, 2), f)
    for k in range(pad.shape[2]):
        S = S + pad[:, :, k]
        Q = pad[:, :, k] * pad[:, :, k] + Q
    S, Q = S[..., 0] + S[..., 1], Q[..., 0] + Q[..., 1]
    S, Q = S[:, 0] + S[:, 1], Q[:, 0] + Q[:, 1]
    S, Q = (S[0] + S[1]) + (S[2] + S[3]), (Q[0] + Q[1]) + (Q[2] + Q[3])
    inv = f(1.0) / f(n)
    mean = S * inv
    var = np.maximum(Q * inv - mean * mean, f(0))
    rstd = f(1.0 / np.sqrt(np.float64(var + f(1e-6))))
    nm = -mean * rstd
    return np.float64((x32 * rstd + nm) * np.asarray(g, f) + np.asarray(e, f))


# ------------------------------------------------------------------ the operand behind a LayerNorm
def operand(y, d, prec, relu):
    """the conv operand r(relu(y)) when the device's y is only known to d -> (base, reach, flip, alt, adjacent): base the rounding of
    the exact y; reach how far the device's operand may lie from it (assertion 1); flip the elements whose roundings of y - d and
    y + d differ; alt their other value; adjacent: every flip is between two neighbouring codes (one tie in the interval)"""
    cut = (lambda v: np.maximum(v, 0.0)) if relu else (lambda v: v)
    lo, hi, base = tw.r_act(cut(y - d), prec), tw.r_act(cut(y + d), prec), tw.r_act(cut(y), prec)
    flip = hi != lo
    alt = np.where(base == lo, hi, lo)
    mid = ((hi + lo) / 2).astype(np.float32)                   # a tie of the format: exact in float32
    below, above = np.nextafter(mid, np.float32(-np.inf)), np.nextafter(mid, np.float32(np.inf))
    adjacent = bool(np.all(~flip | ((tw.r_act(below, prec) == lo) & (tw.r_act(above, prec) == hi))))
    return base, np.maximum(np.abs(hi - base), np.abs(lo - base)), flip, alt, adjacent


def cap(width):
    return min(tw.MAX_FLIPS, int(CAP_SHARE * width))


def _share(got, ref, bd):
    err = np.abs(np.asarray(got, np.float64) - ref)
    return float(np.max(np.where(bd > 0, err / np.where(bd > 0, bd, 1), np.where(err > 0, np.inf, 0.0)))), float(err.max())


# ------------------------------------------------------------------ the three nets and the six sites
def _f64(sd, name):
    return np.asarray(sd[name], np.float64)


@functools.lru_cache(None)
def _fixed(what, C=0):
    """the tensors that are the same in every net (read only, one array each: a caller that keeps a network sets them once)"""
    if what == "identity":
        return tw.identity_conv(C)
    if what == "grid conv2":
        rng = np.random.default_rng(SEED + 5)
        return tw.dyadic(rng, (73, hr.HEAD, 1, 1), -3, 3, 8), tw.dyadic(rng, 73, -8, 8, 4)
    if what == "fc1":                    # unit j adds feature channels j and j + 128, at one pixel each
        j = np.arange(128)
        W1 = np.zeros((128, 64 * hr.HEAD + 7), np.float32)
        W1[j, j * 64 + (7 * j + 3) % 64] = 1.0
        W1[j, (j + 128) * 64 + (11 * j + 5) % 64] = 1.0
        return W1
    return np.zeros(what, np.float32)    # a shape


def _row_conv(sd, name, x):
    sd[name + ".weight"], sd[name + ".bias"] = _fixed(sd[name + ".weight"].shape), np.asarray(x, np.float32)


def _lifted(sd, name, lift):
    sd[name + ".bias"] = tr.bf16_rne(sd[name + ".bias"] + np.float32(lift))


@functools.lru_cache(None)
def base(nb, C, prec, kind):
    """the natural weights a probe net starts from: the same arrays in every net of its kind (read only)"""
    return tw.natural(nb, C, SEED + "sab".index(kind), prec)


class Net:
    """one probe net for one row r = (m, sign, log2 s): `sd`, `nb` blocks, `skip` (the conv biases that carry a row: any float32),
    and its sites"""

    def __init__(self, kind, C, prec, r):
        self.kind, self.C, self.prec, self.r = kind, C, prec, r
        self.nb = 0 if kind == "s" else 1
        self.wprec = "bf16" if prec == "fp32" else prec          # the oracle's fp32 mode runs the bf16 nets unrounded
        sd = self.sd = dict(base(self.nb, C, self.wprec, kind))
        self.x = {}
        bias = {"stem": "conv_block.0", "pln1": "policy_head.model.0", "ln1": "res_blocks.0.conv1", "ln2": "res_blocks.0.conv2",
                "p73": "policy_head.model.2", "vln": "value_head.conv.0"}
        for s in NETS[kind]:
            self.x[s] = row(len(sd[bias[s] + ".bias"]), *r)
            _row_conv(sd, bias[s], self.x[s])
        self.skip = tuple(bias[s] + ".bias" for s in NETS[kind])
        p = "res_blocks.0."
        if kind == "s":
            _lifted(sd, "conv_block.1", LIFT)
            sd["policy_head.model.1.bias"] = np.zeros(hr.HEAD, np.float32)
            sd["policy_head.model.2.weight"], sd["policy_head.model.2.bias"] = _fixed("grid conv2")
        else:
            self.kap = tw.kappa(C, 41)
            tw.constant_layer(sd, "conv_block.1", self.kap)
            tw.transparent_se(sd, C, 0)
            _lifted(sd, p + "bn2", LIFT)
        if kind == "a":
            sd[p + "conv2.weight"], sd[p + "conv2.bias"] = _fixed("identity", C), np.zeros(C, np.float32)
        if kind == "b":
            tw.constant_layer(sd, p + "bn1", tw.kappa(C, 42))
            _lifted(sd, "value_head.conv.1", LIFT)
            j = np.arange(128)
            y, _ = tw.ln(self.x["vln"], _f64(sd, "value_head.conv.1.weight"), _f64(sd, "value_head.conv.1.bias"))
            f = tw.r_act(np.maximum(y, 0), "bf16")
            w2 = np.zeros(128)
            w2[np.argsort(-(f[:128] + f[128:]), kind="stable")] = np.where(j % 2 == 0, 1, -1) / 32.0      # the signs alternate down the sorted sums
            sd["value_head.ffn.0.weight"], sd["value_head.ffn.0.bias"] = _fixed("fc1"), np.zeros(128, np.float32)
            sd["value_head.ffn.2.weight"], sd["value_head.ffn.2.bias"] = w2.astype(np.float32).reshape(1, 128), np.full(1, B2, np.float32)
            self.w2 = w2
        fmt = self.wprec
        for s, ln in (("ln1", p + "bn1"), ("vln", "value_head.conv.1"), ("pln1", "policy_head.model.1")):
            if s in NETS[kind]:          # behind a rounding: the bias puts every exact output on a code of the operand format
                g, e = _f64(sd, ln + ".weight"), _f64(sd, ln + ".bias")
                y = tw.ln(self.x[s], g, e)[0]
                want = {"ln1": np.where(y > 0, tw.r_act(y + 1, fmt), y - 0.5), "vln": tw.r_act(y, "bf16"),
                        "pln1": np.copysign(tw.r_act(np.abs(y) + 1, fmt), y)}[s]
                sd[ln + ".bias"] = (e + (want - y)).astype(np.float32)
                self.skip += (ln + ".bias",)
        self.meta = hr.metas(4)[[0, 3]]                          # both values of meta[0]
        self.sites = [Site(self, s) for s in NETS[kind]]
        b = base(self.nb, C, self.wprec, kind)
        self.unchanged = tuple(n for n, a in sd.items() if a is b.get(n))        # checked once on the base (`check_representable`)

    def check_representable(self):
        tw.representable(self.sd, self.wprec, self.skip + self.unchanged)

    def boards(self):
        """two differing inputs: the probes remove the input"""
        b = np.zeros((2, 8, 8, 112), np.int8)
        b[1, ::2, 1::3, ::5] = 1
        return b


class Site:
    """one LayerNorm of a Net in front of which the row stands: `ln()` the exact value and the one-pass bound, `behind()` the closed
    form from its output (or operand) to what is observed, `check1` / `check2` the two assertions on what is observed: a row [C] of
    the stage (every pixel of every position shows it), the log-probabilities [4672] or the values [2]"""
    OBSERVED = {"stem": "stage", "ln1": "stage", "ln2": "stage", "p73": "logp", "pln1": "logp", "vln": "value"}
    LN = {"stem": "conv_block.1", "ln1": "res_blocks.0.bn1", "ln2": "res_blocks.0.bn2", "p73": "policy_head.model.3",
          "pln1": "policy_head.model.1", "vln": "value_head.conv.1"}

    def __init__(self, net, name):
        self.net, self.name, self.x = net, name, net.x[name]
        self.kind = self.OBSERVED[name]
        self.rounded = name in ("ln1", "vln", "pln1")
        self.relu = name in ("stem", "ln1", "vln")
        self.fmt = net.prec if name != "vln" or net.prec == "fp32" else "bf16"       # the feature row is bf16 at both precisions
        self.g, self.e = _f64(net.sd, self.LN[name] + ".weight"), _f64(net.sd, self.LN[name] + ".bias")
        self.k = dict(k_s=hr.K_LN_S73, k_inv=1) if name == "p73" else {}

    def label(self):
        return f"{self.net.C} {self.net.prec} {self.name} {label(self.net.r)}"

    def ln(self):
        """-> (y, d): the float64 two-pass LayerNorm of the row, and the one-pass fp32 bound on the device's"""
        return tw.ln(self.x, self.g, self.e, **self.k)

    def behind(self, a, da, oracle=False, loose=False):
        """what is observed for LayerNorm outputs (fp32 sites) or operands (sites behind a rounding) a[..., width] whose device copy
        is off by at most da -> (value, bound).  oracle: the oracle's order of the FC2 sum, and of conv2's sum in its fp32 mode.
        loose: the operands are off the operand grid, conv2's sum is not exact (the caller wants the value alone)"""
        sd, n = self.net.sd, self.name
        a = np.asarray(a, np.float64)
        da = np.broadcast_to(np.asarray(da, np.float64), a.shape)
        if n == "stem":
            return np.maximum(a, 0), da
        if n in ("ln1", "ln2"):
            if n == "ln1":
                a, da = tw.ln(a, _f64(sd, "res_blocks.0.bn2.weight"), _f64(sd, "res_blocks.0.bn2.bias"), da)
            return tw.epilogue(a, da, tw.HALF[0], tw.HALF[1], np.float64(self.net.kap), 0.0)
        if n == "vln":
            h, dh = a[..., :128] + a[..., 128:], da[..., :128] + da[..., 128:]
            p = (np.zeros((128, 7)), np.zeros(128), self.net.w2, B2)
            rm = self.net.prec != "fp32"
            lead = h.shape[:-1]
            out = np.empty(lead + (len(self.net.meta),)), np.empty(lead + (len(self.net.meta),))
            for i in np.ndindex(*lead):
                f = np.broadcast_to(h[i], (len(self.net.meta), 128))
                out[0][i] = tr.value_closed(self.net.meta, *p, round_meta=rm, feat=f)
                out[1][i] = tr.value_bound(self.net.meta, *p, k_fc2=tr.K_FC2_ORACLE if oracle else tr.K_FC2_DEVICE, round_meta=rm, feat=f) \
                    + (np.abs(self.net.w2) * dh[i]).sum()          # tanh is 1-Lipschitz
            return out
        if n == "pln1":
            W, b = _f64(sd, "policy_head.model.2.weight").reshape(73, -1), _f64(sd, "policy_head.model.2.bias")
            absum = np.abs(b) + (np.abs(a) + da) @ np.abs(W).T
            z, dz = b + a @ W.T, da @ np.abs(W).T
            if self.net.prec == "fp32":                          # the oracle's own sequential float32 sum
                dz = dz + np.reshape([hr._seq_err(np.concatenate([b[:, None], r[None, :] * W], axis=1)) for r in a.reshape(-1, a.shape[-1])], z.shape)
            elif da.any() or loose:                              # off the grid: any order of 256 products and additions, 2 U each
                dz = dz + 2 * U * (W.shape[1] + 1) * absum
            else:
                hr._exact(self.label() + " conv2", absum, 2.0 ** -14 if self.fmt == "bf16" else 2.0 ** -12)
            a, da = tw.ln(z, _f64(sd, "policy_head.model.3.weight"), _f64(sd, "policy_head.model.3.bias"), dz, k_s=hr.K_LN_S73, k_inv=1)
        lead = a.shape[:-1]
        out = np.empty(lead + (4672,)), np.empty(lead + (4672,))
        for i in np.ndindex(*lead):
            zz, dd = np.repeat(a[i], 64), np.repeat(da[i], 64)
            out[0][i], out[1][i] = tr.logp_closed_z(zz), tr.logp_bound_z(zz, dd)
        return out

    def observe(self, y_ln):
        """what a network whose LayerNorm gives y_ln (float64 of a float32 row) would show at this site, the rest of it exact"""
        if self.rounded and self.net.prec != "fp32":
            y_ln = tw.r_act(np.maximum(y_ln, 0) if self.relu else y_ln, self.fmt)
        return self.behind(y_ln, 0.0, loose=True)[0]

    def check1(self, got, oracle=False):
        """assertion 1 -> (share of the bound used, largest error, the bound's largest element)"""
        assert np.isfinite(got).all(), self.label()
        y, d = self.ln()
        if self.rounded and self.net.prec != "fp32":
            y, d = operand(y, d, self.fmt, self.relu)[:2]
        elif self.rounded and self.relu:
            y = np.maximum(y, 0)
        ref, bd = self.behind(y, d, oracle)
        return _share(got, ref, bd) + (float(bd.max()),)

    def oracle_ln_bound(self):
        """the oracle's own LayerNorm: float64 statistics, then (float)(x - m), * rstd, * g, + e in float32"""
        y = self.ln()[0]
        return 4 * U * np.abs(y - self.e) + U * np.abs(y)

    def check2(self, got, oracle=False):
        """assertion 2 -> (share of the tolerance used; inf where the row has more elements on a tie than `cap`, largest error,
        the largest |exact|, elements excused).  oracle: the elements excused are those within the ORACLE's LayerNorm error of a
        tie (it is two-pass at every rung), and the oracle's order of the FC2 sum"""
        y, d = self.ln()
        if oracle:
            d = self.oracle_ln_bound()
        if self.net.prec == "fp32":          # the oracle's fp32 mode: no operand; its own LayerNorm is float32 arithmetic on float64 statistics
            ref, bd = self.behind(np.maximum(y, 0) if self.rounded and self.relu else y, d, oracle=True)
            if not self.rounded:
                bd = self._tol(y, ref, "bf16")
            return _share(got, ref, bd) + (float(np.abs(ref).max()), 0)
        if not self.rounded:
            ref = self.behind(y, 0.0, oracle)[0]
            return _share(got, ref, self._tol(y, ref, self.fmt)) + (float(np.abs(ref).max()), 0)
        base, _, flip, alt, adjacent = operand(y, d, self.fmt, self.relu)
        idx = np.flatnonzero(flip)
        if len(idx) > cap(len(y)) or not adjacent:               # too many on a tie: none is excused
            idx = idx[:0]
        A = np.repeat(base[None], 2 ** len(idx), 0)
        for v, bits in enumerate(itertools.product((0, 1), repeat=len(idx))):
            A[v, idx[np.flatnonzero(bits)]] = alt[idx[np.flatnonzero(bits)]]
        ref, bd = self.behind(A, 0.0, oracle)
        sh = [_share(got, r, b) for r, b in zip(ref, bd)]
        return min(sh) + (float(np.abs(ref[0]).max()), len(idx))

    def _tol(self, y, ref, fmt):
        if self.name != "p73":
            return operand_tol(ref, fmt)
        return self.behind(y, operand_tol(y, fmt))[1]          # on the LayerNorm's own output, carried through the log-softmax


def one_row(got, kind):
    """a stage [n,64,C], log-probabilities [n,4672] or values [n] of a Net -> the one row / vector that every pixel and every position
    must show, after asserting that they do (values: per meta row)"""
    got = np.asarray(got)
    if kind == "stage":
        flat = (got.reshape(-1, got.shape[-1]) + np.float32(0)).view(np.uint32)
        assert (flat == flat[0]).all(), "pixels or positions differ"
        return np.float64(got[0, 0])
    if kind == "logp":
        assert (got == got[0]).all() and (got[0].reshape(73, 64) == got[0].reshape(73, 64)[:, :1]).all(), "pixels or positions differ"
        return np.float64(got[0])
    return np.float64(got)


def first_failing(shares):
    """{(m, sign, log2 s): share of assertion 2} -> the first rung m with a share above 1 (None: no rung fails)"""
    bad = sorted({r[0] for r, s in shares.items() if not s <= 1.0})
    return bad[0] if bad else None


# ------------------------------------------------------------------ R_REQ: mean / sigma of the project's own networks
LN_SITES = ("stem", "ln1", "ln2", "pln1", "p73", "vln")
NETWORKS = (("1 x 256", 1, 256, "nn_ref_b1_c256"), ("10 x 256", 10, 256, "nn_ref_b10_c256"), ("19 x 256", 19, 256, "nn_ref_b19_c256"),
            ("20 x 256", 20, 256, "nn_ref_b20_c256"), ("10 x 128", 10, 128, "nn_ref_b10_c128"),
            ("10 x 256 g4v2 (trained magnitudes)", 10, 256, "nn_ref_b10_c256_sharp"), ("10 x 256 g8", 10, 256, "nn_ref_b10_c256_sharp"))


# what `measure_ratios` gives, to three decimals, in the order of LN_SITES (DESIGN.md section 7 repeats it)
RATIOS = {
    "1 x 256": (0.176, 0.173, 0.148, 0.208, 0.357, 0.124),
    "10 x 256": (0.231, 0.197, 0.251, 0.121, 0.221, 0.132),
    "19 x 256": (0.233, 0.241, 0.216, 0.194, 0.202, 0.177),
    "20 x 256": (0.190, 0.218, 0.209, 0.135, 0.136, 0.092),
    "10 x 128": (0.212, 0.338, 0.272, 0.102, 0.173, 0.218),
    "10 x 256 g4v2 (trained magnitudes)": (0.153, 0.233, 0.229, 0.080, 0.247, 0.145),
    "10 x 256 g8": (0.153, 0.233, 0.229, 0.080, 0.247, 0.145),
}


def measure_ratios(orc, gold_dir, networks=NETWORKS):
    """-> {network: {site: the largest per-pixel |mean| / sqrt(var + 1e-6) of the LayerNorm's input}}: float64 statistics of the
    oracle's fp32 mode (orc.Net.ln_ratios) over every distinct position of the nn_ref_* goldens, golden_boards() among them; each
    network on the seed of its golden.  The sharp recipes scale a LayerNorm gain and FC2, which no LayerNorm input sees: their rows
    repeat the seed's"""
    import glob
    import os

    import sharp_nets
    pos = {}
    for f in sorted(glob.glob(os.path.join(gold_dir, "nn_ref_*.npz"))):
        g = np.load(f)
        pos.update({b.tobytes() + m.tobytes(): (b, m) for b, m in zip(g["boards"], g["meta"])})
    out = {}
    for name, nb, C, gold in networks:
        seed = int(np.load(os.path.join(gold_dir, gold + ".npz"))["seed"])
        kind = [k for k in sharp_nets.KINDS if k in name]
        net = sharp_nets.oracle_net(orc, nb, C, seed, kind[0]) if kind else orc.Net(nb, C, seed=seed)
        r = np.max([net.ln_ratios(b, m) for b, m in pos.values()], axis=0)
        blk = r[1:1 + 2 * nb].reshape(nb, 2).max(0)
        out[name] = dict(zip(LN_SITES, (r[0], blk[0], blk[1], r[-3], r[-2], r[-1])))
    return out


def required_rung(largest):
    """the next rung at or above 8 times the largest ratio"""
    return min(m for m in RUNGS if m >= 8 * largest)


# ------------------------------------------------------------------ the CPU checks (tests/test_tower_ref.py, tests/test_heads_ref.py)
MODES = {"fp32": {}, "bf16": {"emulate_bf16": True}, "fp8": {"emulate_fp8": True}}


def kinds_of(sites):
    return [k for k, ss in NETS.items() if set(ss) & set(sites)]


def oracle_observed(cache, orc, net):
    """what the oracle makes of a Net -> {"stage": row [C], "logp": [4672], "value": [2]}; cache: a dict that keeps one oracle
    network per shape and sets only the tensors that changed"""
    key = (net.kind, net.C, net.prec)
    if key not in cache:
        cache[key] = (orc.Net(net.nb, net.C, seed=1, **MODES[net.prec]), {})
    onet, cur = cache[key]
    for i, (name, _, _, _) in enumerate(scw.tensor_table(net.nb, net.C)):
        if cur.get(name) is not net.sd[name]:
            onet.set_tensor(i, net.sd[name])
            cur[name] = net.sd[name]
    res = [onet.forward(b, m, latent=True) for b, m in zip(net.boards(), net.meta)]
    return {"stage": one_row(np.stack([r[2] for r in res]), "stage"), "logp": one_row(np.stack([r[0] for r in res]), "logp"),
            "value": one_row(np.asarray([r[1] for r in res], np.float32), "value")}


def check_oracle(orc, C, prec, sites):
    """the oracle (two-pass in double) on every row: assertion 1 and assertion 2 on EVERY rung, at the sites named"""
    cache, top = {}, {s: [0.0, 0.0] for s in sites}
    for kind in kinds_of(sites):
        tw.representable(base(0 if kind == "s" else 1, C, "bf16" if prec == "fp32" else prec, kind), "bf16" if prec == "fp32" else prec)
    for r in rows():
        for kind in kinds_of(sites):
            net = Net(kind, C, prec, r)
            net.check_representable()
            got = oracle_observed(cache, orc, net)
            for st in net.sites:
                if st.name in sites:
                    s1, s2 = st.check1(got[st.kind], oracle=True), st.check2(got[st.kind], oracle=True)
                    top[st.name] = [max(top[st.name][0], s1[0]), max(top[st.name][1], s2[0])]
                    assert s1[0] <= 1 and s2[0] <= 1, (st.label(), s1, s2)
    for s, (a, b) in top.items():
        print(f"oracle {C} {prec} {s}: {len(rows())} rows; largest share of the one-pass bound {a:.3g}, of assertion 2's tolerance {b:.3f}")


def wrong_ln_shares(C, prec, site):
    """the net whose LayerNorm at `site` is one_pass32 and whose every other layer is exact -> {row: (share of 1, share of 2)}"""
    kind = kinds_of([site])[0]
    out = {}
    for r in rows():
        st = [s for s in Net(kind, C, prec, r).sites if s.name == site][0]
        got = st.observe(one_pass32(st.x, st.g, st.e))
        out[r] = (st.check1(got)[0], st.check2(got)[0])
    return out


def check_wrong_ln(C, prec, site):
    """the one-pass LayerNorm stays within assertion 1 on every rung, meets 2 on every rung below its break rung and fails it on
    that rung and on every rung above; the break rung lies above R_REQ -> the break rung"""
    sh = wrong_ln_shares(C, prec, site)
    assert all(a <= 1 for a, _ in sh.values()), (site, C, prec, {label(r): a for r, (a, _) in sh.items() if a > 1})
    brk = first_failing({r: b for r, (_, b) in sh.items()})
    print(f"one-pass fp32 LayerNorm at {C} {prec} {site}: first rung failing assertion 2: {brk}; shares of its tolerance by row: "
          + ", ".join(f"{label(r)}: {b:.3g}" for r, (_, b) in sh.items()))
    assert brk is not None and brk > R_REQ, (site, C, prec, brk)
    assert all(b <= 1 for r, (_, b) in sh.items() if r[0] < brk)
    assert all(any(b > 1 for r, (_, b) in sh.items() if r[0] == m) for m in RUNGS if m >= brk)
    return brk


def check_conditions(C, prec, sites):
    """the probes' own conditions, no network in the loop: every row exact in float32 (`row` asserts it); no ReLU cut where the lift is
    meant to prevent it; behind a rounding, the float64 reference alone excuses at most `cap` elements on every rung up to R_REQ,
    and a single wrong operand (the other neighbour of one element) moves the output by at least MIN_MOVE bounds"""
    for r in rows():
        for kind in kinds_of(sites):
            net = Net(kind, C, prec, r)
            for st in net.sites:
                if st.name not in sites:
                    continue
                y, d = st.ln()
                if st.name in ("stem", "ln2", "vln"):
                    assert y.min() > 1.0, (st.label(), y.min())
                if st.name in ("ln2", "ln1"):
                    assert st.behind(tw.r_act(np.maximum(y, 0), prec) if st.rounded else y, 0.0)[0].min() > 0.5
                if st.name == "pln1":
                    assert 1 <= np.abs(y).min() and np.abs(y).max() < 4
                if st.rounded and r[0] <= R_REQ:
                    base_, _, flip, _, adjacent = operand(y, d, st.fmt, st.relu)
                    assert flip.sum() == 0 <= cap(len(y)) and adjacent, (st.label(), int(flip.sum()))     # on a code: none at all
                    live = np.flatnonzero(base_ != 0)
                    A = np.repeat(base_[None], len(live), 0)
                    A[np.arange(len(live)), live] += 2 * half_ulp(base_[live], st.fmt)
                    (r0, b0), (r1, _) = st.behind(base_, 0.0), st.behind(A, 0.0, loose=True)
                    move = (np.abs(r1 - r0) / b0).max(-1).min()
                    assert move >= MIN_MOVE, (st.label(), move)


MIN_MOVE = 4               # a single operand one step off moves some output element by at least this many of its bounds
