"""The yardstick of the output-tail tests: probe weights that make the tail's input known exactly, the closed forms of what the tail
must then compute (float64 numpy on the weights alone), and the error bounds the oracle and the GPU results are held to.

The tail (csrc/nn_tower32.hpp, "log_softmax over 4672" to the end; csrc/value_tail.hpp) is the only float arithmetic whose results go
straight into the search tree: log-softmax over the 4672 actions, the legal-move priors exp(logp[idx]) / (sum + 1e-5)
(src/backends/torch.rs:148-175, src/chess.rs:891), and the value tail (meta as bf16, FC1 bias + 7 meta columns, ReLU, FC2, tanh, sign).

PROBES.  `policy_probe` zeroes the gain of the policy head's last LayerNorm and sets its bias to b[73]: `t * 0 + b` is b exactly, so the
logit of action ch*64 + px (the flatten is channel-major) is b[ch] for every pixel and every input.  `value_probe` zeroes the 64*256
feature columns of value_head.ffn.0: the split-K partials are exact zeros and the value depends on meta alone.  Every probe value must
survive a bfloat16 round trip (asserted), so nothing is assumed about which tensors the engine rounds at load.

BOUNDS, first order in U = 2^-24 (the unit roundoff of float32): K roundings x U plus one term per hardware function, computed from the
data as tests/score_ref.py does.  The models of the functions (confirmed by the measured maxima that the tests print):
  * `__expf(x)` is `v_mul_f32 x, log2(e)` feeding `v_exp_f32`, with no range scaling in between -- seen in the gfx950 assembly of
    nn_kernels.hip and step_kernels.hip (hipcc -S, device only): every exponential of the softmax and of the prior gather is
    `v_sub_f32; v_mul_f32 0x3fb8aa3b, x; v_exp_f32`, no v_cmp / v_ldexp around it.  The hardware 2^y is taken at 1 ulp (2^-23 relative);
    the rounded product moves y by |x| log2(e) U, which 2^y turns into a relative error of the same size -- modelled, with the rounding
    of the constant, as EXP(x) = 2^-23 + |x| log2(e) 2^-23 (twice the product-rounding term).
  * `__logf(s)` does NOT lower to a bare `v_log_f32` times ln 2, as first assumed: the assembly shows the full logf expansion
    (v_cmp / v_ldexp scaling of denormal arguments, v_log_f32, then the product with ln 2 as a high and a low word, 0x3f317217 and
    0x3377d1cf, through v_fma).  That is more accurate than the assumed lowering, so the model keeps the assumed one as its upper
    bound: 1 ulp of the hardware, one product rounding, the rounded constant: LOG_REL = 2^-23 + 2 U relative to |ln s|, plus
    ln 2 * 2^-24 absolute (the hardware's error near s = 1 is absolute in log2).
  * The 4-way combine compiles to v_mul + v_fmac per pair (contraction is on in these two files): one rounding fewer per pair than
    the count below, which stays an upper bound.
  * `tanhf` is the library function: 2 ulp (HIP math-function table, single precision), TANH_REL = 2^-22 relative."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
LOG_REL = 2.0 ** -23 + 2 * U
TANH_REL = 2.0 ** -22
EPS_PRIOR = float(np.float32(1e-5))    # the float32 constant of post_process_distr (src/chess.rs:891)
K_SE = 18 + 6 + 1 + 2                  # per-lane 19-term sum, wave_sum_fixed (4 DPP levels + 2), rescale product, 4-way combine
K_PRIOR_SUM = 6 + 2 + 1                # wave_sum_fixed, the four wave sums pairwise, + 1e-5
K_FC1 = 14                             # bias + 7 meta products: 7 product roundings, 7 additions
K_FC2_DEVICE = 3 + 6 + 1               # the lane's pair (2 products, 1 addition), wave_sum_fixed, + fc2 bias
K_FC2_ORACLE = 1 + 128                 # oracle/nn.c: one product and a sequential float32 sum of 128 terms behind the bias
CEIL_LOGP = 1e-4                       # at |logp| <= 40: today's row-normalisation check; a looser bound would add nothing
CEIL_PRIOR = 1e-4                      # relative

PLANES = 73
WIDTHS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 217, 218)
FEN218 = "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - %d %d"   # 218 legal moves in 23 move planes; fields: halfmove, fullmove


def bf16_rne(x):
    """float32 -> the nearest bfloat16 (as float32), ties to even: the rounding of value_tail.hpp and oracle/nn.c"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def _assert_bf16(name, a):
    a = np.asarray(a, np.float32)
    assert np.array_equal(bf16_rne(a).view(np.uint32), a.view(np.uint32)), f"{name}: not representable in bfloat16"


# ------------------------------------------------------------------ probes
def policy_probe(sd, b):
    """in place: gain 0 and bias b[73] in the policy head's last LayerNorm -- every logit of plane ch is b[ch]"""
    b = np.asarray(b, np.float64)
    assert b.shape == (PLANES,)
    _assert_bf16("policy bias", b)
    assert np.array_equal(np.float32(b).astype(np.float64), b)
    sd["policy_head.model.3.weight"] = np.zeros(PLANES, np.float32)
    sd["policy_head.model.3.bias"] = b.astype(np.float32)
    return sd


def value_probe(sd, Wm, b1, w2, b2):
    """in place: value_head.ffn.0 keeps only its 7 meta columns Wm[128][7] and bias b1[128]; ffn.2 is w2[128], b2"""
    Wm, b1, w2 = np.asarray(Wm, np.float64), np.asarray(b1, np.float64), np.asarray(w2, np.float64)
    assert Wm.shape == (128, 7) and b1.shape == (128,) and w2.shape == (128,)
    for name, a in (("Wm", Wm), ("b1", b1), ("w2", w2), ("b2", [b2])):
        _assert_bf16(name, a)
    W = np.zeros_like(sd["value_head.ffn.0.weight"])
    assert W.shape == (128, 64 * 256 + 7)
    W[:, 64 * 256:] = Wm
    sd["value_head.ffn.0.weight"] = W
    sd["value_head.ffn.0.bias"] = b1.astype(np.float32)
    sd["value_head.ffn.2.weight"] = w2.astype(np.float32).reshape(1, 128)
    sd["value_head.ffn.2.bias"] = np.asarray([b2], np.float32)
    return sd


def wave_of_plane(ch):
    """thread = action % 256 and action = ch*64 + px: move plane ch is reduced by wave ch % 4 of the softmax"""
    return ((np.asarray(ch) * 64) % 256) // 64


def _levels():
    q = (np.arange(PLANES) * 37) % PLANES                 # a permutation of 0..72 (37 and 73 are coprime): no monotone plane order
    return 0.25 * np.rint(q * 128 / 72.0)                 # 73 distinct multiples of 0.25 in [0, 32], 0 and 32 among them


def bias_patterns():
    """name -> b[73] (float64).  `levels` lies in [0, 32] so that every pattern, `low` = levels - 64 included, is made of
    bfloat16 values (multiples of 0.25 up to 64, of 0.5 up to 128)"""
    lv = _levels()
    pats = {"flat": np.zeros(PLANES), "levels": lv}
    for w in range(4):
        pats[f"wave{w}"] = lv + 24.0 * (np.arange(PLANES) % 4 == w)     # maximum and mass in one wave's share
    far = lv - 32.0
    far[42] = 96.0                                        # wave 2; the other waves' rescale factors exp(m_w - 96) underflow
    pats["far"] = far
    pats["low"] = lv - 64.0                               # the closed form is that of `levels` exactly (shift invariance)
    return pats


FULLMOVES = (1, 2, 255, 256, 257, 259, 301, 303, 511, 513, 1023)
HALFMOVES = (0, 1, 99, 100, 127, 149)
CASTLING = ((0, 0, 0, 0), (1, 1, 1, 1), (1, 0, 1, 0), (0, 1, 0, 1))


def meta_grid(n=130, seed=11):
    """n rows of the turn x fullmove x halfmove x castling grid (528 cells), every value of every factor among them"""
    cells = [(t, f) + c + (h,) for t in (0, 1) for f in FULLMOVES for h in HALFMOVES for c in CASTLING]
    pick = np.random.default_rng(seed).permutation(len(cells))[:n]
    m = np.asarray([cells[i] for i in pick], np.int32)
    assert set(m[:, 0]) == {0, 1} and set(m[:, 1]) == set(FULLMOVES) and set(m[:, 6]) == set(HALFMOVES)
    assert {tuple(r) for r in m[:, 2:6]} == set(CASTLING)
    return m


def value_probes():
    """name -> (Wm, b1, w2, b2).  `spread`: units that grow with the fullmove number pull s up, units that grow with the halfmove
    clock pull it down, so s covers (-2.8, 2.8) over the meta grid (tests/test_tail_ref.py asserts the range); `saturated`: the
    same first layer with w2 >= 0 and b2 = 14, so s >= 12 and |v| = 1 to within one ulp"""
    r = np.random.default_rng(6)
    Wm = np.zeros((128, 7))
    Wm[:, 0] = r.integers(-32, 33, 128) / 64.0            # turn
    Wm[:, 1] = r.integers(-3, 4, 128) / 128.0             # fullmove (up to 1023, 1024 as bfloat16)
    Wm[:, 2:6] = r.integers(-32, 33, (128, 4)) / 64.0     # castling bits
    Wm[:, 6] = r.integers(-3, 4, 128) * 6 / 128.0         # halfmove clock (up to 149)
    b1 = r.integers(-64, 65, 128) / 64.0
    w2 = (np.sign(Wm[:, 1]) - np.sign(Wm[:, 6]) + r.integers(-1, 2, 128)) * r.integers(1, 4, 128) / 512.0
    return {"spread": (Wm, b1, w2, 0.0), "saturated": (Wm, b1, np.abs(w2), 14.0)}


# ------------------------------------------------------------------ closed forms
def logp_closed(b):
    """float64 [4672]: logp[ch*64 + px] = b[ch] - log(64 * sum_c exp b[c])"""
    b = np.asarray(b, np.float64)
    mx = b.max()
    lse = mx + np.log(64.0 * np.exp(b - mx).sum())
    return np.repeat(b - lse, 64)


def _fc(meta, Wm, b1, w2, b2, round_meta, feat=None):
    """feat: the feature columns' share of FC1, [n][128] (tests/heads_ref.py); None where the probe zeroes those columns"""
    meta = np.asarray(meta, np.int32).reshape(-1, 7)
    m = np.asarray(bf16_rne(meta.astype(np.float32)) if round_meta else meta, np.float64)
    h = np.asarray(b1, np.float64)[None, :] + m @ np.asarray(Wm, np.float64).T
    if feat is not None:
        h = h + np.asarray(feat, np.float64)
    a = np.abs(np.asarray(b1, np.float64))[None, :] + np.abs(m) @ np.abs(np.asarray(Wm, np.float64)).T
    r = np.maximum(h, 0.0)
    s = r @ np.asarray(w2, np.float64) + b2
    return meta, a, r, s


def value_closed(meta, Wm, b1, w2, b2, round_meta=True, feat=None):
    """float64 [n]: tanh(sum_j relu(b1[j] + feat[j] + sum_k bf16(meta[k]) Wm[j][k]) w2[j] + b2) (2 turn - 1).  round_meta=False is
    the oracle's fp32 mode, which feeds meta unrounded (oracle/nn.c rounds it in the emulating modes only)"""
    meta, _, _, s = _fc(meta, Wm, b1, w2, b2, round_meta, feat)
    return np.tanh(s) * (2.0 * meta[:, 0] - 1.0)


def priors_from_logp(logp_row_f32, idx):
    """the reference's own definition, exp(lp[idx]) / (sum + float32(1e-5)), in float64: on the float32 log-probabilities an engine
    returns (converted exactly) or on a float64 closed form"""
    e = np.exp(np.asarray(logp_row_f32, np.float64)[np.asarray(idx, np.int64)])
    return e / (e.sum() + EPS_PRIOR)


# ------------------------------------------------------------------ bounds
def exp_rel(x):
    """relative error of __expf at argument x (module docstring)"""
    return 2.0 ** -23 + np.abs(x) * LOG2E * 2.0 ** -23


def logp_bound(b):
    """float64 [4672]: |device logp - logp_closed(b)| per action: logp_bound_z of the logits b[ch] at every pixel"""
    return logp_bound_z(np.repeat(np.asarray(b, np.float64), 64))


def logp_closed_z(z):
    """float64 [4672]: z - log sum exp z"""
    z = np.asarray(z, np.float64)
    mx = z.max()
    return z - (mx + np.log(np.exp(z - mx).sum()))


def logp_bound_z(z, dz=0.0):
    """float64 [4672]: |device logp - logp_closed_z(z)| per action, for logits whose device copy is off by at most dz (elementwise:
    its own dz, plus the t-weighted mean of dz through the sum of exponentials).  Terms, for exact logits z (wave w = plane % 4 holds
    maximum m_w, mx = max m_w, t_i = exp(z_i - mx)):
      se     relative error of the sum of exponentials = the t-weighted mean of
             [ z_i - m_w rounded (|z_i - m_w| U) + EXP(z_i - m_w)               the lane's exponential
             + 18 U (per-lane 19-term sum) + 6 U (wave_sum_fixed)
             + m_w - mx rounded + EXP(m_w - mx) + 1 U (rescale product) + 2 U    the 4-way rescale and combine ]
             plus 2 * 4672 * 2^-126 / se for exponentials and products that underflow
      log    |ln se| LOG_REL + ln 2 * 2^-24
      lse    mx + log(se): |lse| U
      z-lse  |logp_i| U"""
    z = np.asarray(z, np.float64)
    dz = np.broadcast_to(np.asarray(dz, np.float64), z.shape)
    wave = (np.arange(4672) % 256) // 64
    mw = np.asarray([z[wave == w].max() for w in range(4)])
    mx = mw.max()
    a, r = np.abs(z - mw[wave]), np.abs(mw[wave] - mx)
    t = np.exp(z - mx)
    se = t.sum()
    e_se = (t * (a * U + exp_rel(a) + r * U + exp_rel(r) + K_SE * U)).sum() / se + 2 * 4672 * TINY / se
    lse = mx + np.log(se)
    return e_se + np.abs(np.log(se)) * LOG_REL + LN2 * U + np.abs(lse) * U + np.abs(z - lse) * U + dz + (t * dz).sum() / se


def prior_bound(logp_row, idx, arg_err=0.0):
    """-> (float64 [n] absolute bound per prior, float64 [n] its relative part) against priors_from_logp(logp_row, idx).
    arg_err: how far the device's own float32 argument s_z - lse may lie from logp_row[idx] (0 where logp_row IS the device's
    logp, logp_bound(b)[idx] against a closed form): exp turns it into a relative error.  Terms:
      own exponential   EXP(lp_i) + arg_err_i
      sum               the largest exponential term max_j (EXP(lp_j) + arg_err_j) + (6 + 2 + 1) U for the tree
      division          1 U (correctly rounded)
    and, absolute, 2^-126 / s for exponentials that underflow"""
    idx = np.asarray(idx, np.int64)
    x = np.asarray(logp_row, np.float64)[idx]
    own = exp_rel(x) + np.broadcast_to(np.asarray(arg_err, np.float64), x.shape)
    rel = own + own.max() + (K_PRIOR_SUM + 1) * U
    e = np.exp(x)
    s = e.sum() + EPS_PRIOR
    return rel * e / s + TINY / s, rel


def value_bound(meta, Wm, b1, w2, b2, k_fc2=K_FC2_DEVICE, round_meta=True, feat=None):
    """float64 [n]: |value - value_closed|.  Terms:
      FC1     14 roundings on |b1_j| + sum_k |m_k Wm_jk| per hidden unit (bias + 7 products, 7 additions; the zero partials add nothing)
      FC2     k_fc2 roundings on sum_j |relu_j w2_j| + |b2|: the lane's pair 3, wave_sum_fixed 6, the bias 1 (oracle: 129, sequential)
      tanh    the error of its argument times 1 - v^2 (taken at the nearer end of the argument's interval), TANH_REL |v| for the
              function, 1 U |v| for the rounding of the result (the sign factor is exact)"""
    _, a, r, s = _fc(meta, Wm, b1, w2, b2, round_meta, feat)
    w2 = np.abs(np.asarray(w2, np.float64))
    e_s = K_FC1 * U * (a @ w2) + k_fc2 * U * (r @ w2 + abs(b2))           # the feature share: every partial sum exact (heads_ref)
    v = np.abs(np.tanh(s))
    slope = 1.0 - np.tanh(np.maximum(np.abs(s) - e_s, 0.0)) ** 2
    return slope * e_s + (TANH_REL + U) * v + TINY


def value_args(meta, Wm, b1, w2, b2, round_meta=True, feat=None):
    """float64 [n]: the argument s of tanh (the tests check the probes' ranges on it)"""
    return _fc(meta, Wm, b1, w2, b2, round_meta, feat)[3]


# ------------------------------------------------------------------ index sets of the prior tests
def index_sets(logp_row, n, rng):
    """name -> n distinct actions: random, the row's top n, its bottom n, and a set that holds the arg-max and the arg-min"""
    order = np.argsort(np.asarray(logp_row, np.float64), kind="stable")
    keep = [order[-1]] if n == 1 else [order[-1], order[0]]
    rest = [i for i in rng.permutation(4672) if i not in keep][:n - len(keep)]
    mixed = rng.permutation(np.asarray(keep + rest, np.int64))
    return {"random": rng.permutation(4672)[:n], "top": rng.permutation(order[-n:]), "bottom": rng.permutation(order[:n]), "mixed": mixed}
