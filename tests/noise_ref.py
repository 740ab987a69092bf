"""The yardstick of the root-noise tests: `mix64`, `sc_rng` (csrc/chess_rules.hpp), `u01_open`, `gamma03` and the normalisation of
the root's Dirichlet(0.3) noise (csrc/search_select.hpp) restated in vectorised numpy, and the error bounds the GPU's samples are held to.
tests/test_noise_ref.py checks this module on the CPU (the law of the draws, the rare paths, the bounds' form).

The replay follows the kernel literally: the same stream order (u0 for the boost, then a, b, u per iteration), NO third uniform when
v <= 0, at most 64 iterations and then `boost * d`, the kernel's f32 constants, its association of every expression, and cos(2 pi b) for
`v_cos_f32`, which takes revolutions.  The uniforms are computed in f32 in every replay, as the kernel computes them ((k + 0.5) rounds for
k >= 2^23): they are the INPUT of the floating-point code under test, not part of its error.

dtype = float64 is the yardstick: the kernel's formula evaluated (nearly) exactly on the kernel's inputs.  dtype = float32 rounds every
operation to f32 and every function correctly (the f64 function of the f32 argument, rounded once): what the kernel would compute if the
hardware's transcendentals were correctly rounded; its sum follows `wave_sum_fixed` (csrc/wave_util.hpp) addition by addition.

Bounds, first order, in U = 2^-24 (the unit roundoff of f32).  A function within e ulps has relative error <= 2 e U (log, exp, sqrt;
e = 1/2 when correctly rounded); the cosine's error is taken ABSOLUTE, <= 2 e U (ulps of 1: near its zeros no relative bound holds and only
the absolute error reaches v).  Per draw, with L0 = log2 u0, r = sqrt(-2 ln a), x = r cos(2 pi b), v1 = 1 + c x (the value that is cubed):

    boost = exp2(fl(L0' / alpha)):            ln 2 * |L0| / alpha * (E_log + U) + E_exp
    x:  |dx| <= |x| (E_log / 2 + U / 2 + E_sqrt + U) + r E_cos         (log, product, sqrt, product; cosine)
    v1: |dv1| / v1 <= (c |dx| + |c x| U) / v1 + U                      (the cancellation in 1 + c x: everything on c x is amplified by 1 / v1)
    value = fl(fl(boost d) fl(fl(v1 v1) v1)): boost + 3 (v1 term) + 4 U

which is affine in the four constants: rel = A + E_log B_log + E_exp B_exp + E_cos B_cos + E_sqrt B_sqrt (`draw_bound`).  Per sample
(`sample_bound`): entry i of g / sum(g) errs relatively by at most its draw's bound, plus the sum's (the draws' bounds weighted by the
draws, plus one U per addition on the longest chain of the fixed-order sum: the lane's own nr - 1 additions, four DPP levels, two
levels over the rows), plus one division.

The accept/reject decisions (`v <= 0`, the squeeze test) are discontinuities: a draw whose smallest decision margin -- |lhs - rhs| of the
acceptance test, |v1| of the sign test, over its iterations, in float64 -- is below MARGIN may legitimately take another branch on the
device, and a sample holding such a draw is FLAGGED: the only samples a comparison may skip."""
import numpy as np

U = 2.0 ** -24
MARGIN = 1e-5            # a draw with a smaller decision margin flags its sample
MAX_FLAGGED = 0.01       # at most this share of the samples of any width may be flagged
HALF_ULP = dict(log=0.5, exp=0.5, cos=0.5, sqrt=0.5)   # correctly rounded functions (the float32 replay)
# The hardware's v_log_f32 / v_exp_f32 / v_cos_f32 / v_sqrt_f32, in ulps.  Only finished samples can be read back from the kernels that
# ship, so the four are measured jointly on the MI355X: the smallest COMMON value at which every unflagged entry of the 12 x 2496 samples
# of tests/test_gpu_noise.py::test_every_sample_equals_the_replay is within the bound was 0.243 (roots of 137; 0.000 .. 0.169 at the other
# widths), committed at twice that.  The figure is what the worst-case sum of the roundings above leaves to the
# functions, not an accuracy figure of one instruction: with it the device's samples are held to the bound of a float32 evaluation
# whose functions are correctly rounded.
HW_ULP = dict(log=0.5, exp=0.5, cos=0.5, sqrt=0.5)

F32 = np.float32
# the kernel's constants: f32 values, folded in f32 by the compiler
ALPHA = F32(0.3)
INV_ALPHA = F32(1.0) / ALPHA
D = F32(F32(ALPHA + F32(1.0)) - F32(F32(1.0) / F32(3.0)))
C_MT = F32(0.3390317518)    # 1 / sqrt(9 d)
LN2 = F32(0.69314718)
M2LN2 = F32(F32(-2.0) * LN2)
MAX_ITER = 64


def mix64(z):
    """splitmix64's finaliser on uint64 arrays (wraps like the C code)"""
    with np.errstate(over="ignore"):
        z = np.asarray(z, np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _u64(x):
    if isinstance(x, np.ndarray):
        return x.astype(np.uint64)
    return np.uint64(int(x) & 0xFFFFFFFFFFFFFFFF)


def sc_rng(seed, game, ply, purpose, counter):
    """the counter RNG's key (csrc/chess_rules.hpp), broadcasting over uint64 arrays"""
    seed, game, ply, purpose, counter = (_u64(a) for a in (seed, game, ply, purpose, counter))
    with np.errstate(over="ignore"):
        h = mix64(seed ^ (game * np.uint64(0xD1B54A32D192ED03)))
        h = mix64(h ^ (ply * np.uint64(0x8CB92BA72F3D8DD7)))
        return mix64(h ^ ((purpose << np.uint64(48)) | counter))


def u01_open(st):
    """(next state, f32 uniform): st = mix64(st); ((float)(st >> 40) + 0.5f) * 2^-24, in f32 like the kernel"""
    st = mix64(st)
    k = (st >> np.uint64(40)).astype(np.float32)       # 24 bits: exact
    return st, (k + F32(0.5)) * F32(1.0 / 16777216.0)  # the sum rounds (to even) from k = 2^23 on; the product is exact


class _Ops:
    """arithmetic in `dtype`; functions exact in float64, correctly rounded in float32"""

    def __init__(self, dtype):
        self.t = np.dtype(dtype).type
        assert self.t in (np.float32, np.float64)

    def fn(self, f, x):
        return f(x.astype(np.float64)).astype(self.t)

    def log2(self, x):
        return self.fn(np.log2, x)

    def exp2(self, x):
        return self.fn(np.exp2, x)

    def sqrt(self, x):
        return self.fn(np.sqrt, x)

    def cos_rev(self, b):
        return self.fn(lambda y: np.cos(2.0 * np.pi * y), b)


def gamma03(st, dtype=np.float64):
    """gamma03(st) of csrc/search_select.hpp for a uint64 array of keys.  -> dict of arrays, per draw:
    value; iters (iterations run, 1..64); cont (iterations left by `v <= 0`); fell (True: 64 iterations without acceptance, the value
    is boost * d); margin (the smallest decision margin met, float64); log2u0, and r, x, v1 of the LAST iteration (what a bound needs)"""
    o = _Ops(dtype)
    t = o.t
    st = np.array(st, np.uint64).reshape(-1)
    n = st.size
    st, u0 = u01_open(st)
    log2u0 = o.log2(u0.astype(t))
    boost = o.exp2(log2u0 * t(INV_ALPHA))
    d, c, ln2 = t(D), t(C_MT), t(LN2)
    value = boost * d                                  # the fall-through after 64 iterations
    iters = np.zeros(n, np.int32)
    cont = np.zeros(n, np.int32)
    margin = np.full(n, np.inf)
    r_out, x_out, v1_out = np.zeros(n, t), np.zeros(n, t), np.ones(n, t)
    act = np.arange(n)
    for _ in range(MAX_ITER):
        if act.size == 0:
            break
        s, a = u01_open(st[act])
        s, b = u01_open(s)
        r = o.sqrt(t(M2LN2) * o.log2(a.astype(t)))
        x = r * o.cos_rev(b.astype(t))
        v1 = t(1.0) + c * x
        iters[act] += 1
        margin[act] = np.minimum(margin[act], np.abs(v1.astype(np.float64)))
        r_out[act], x_out[act], v1_out[act] = r, x, v1
        pos = v1 > 0
        cont[act[~pos]] += 1
        st[act[~pos]] = s[~pos]                        # `continue`: no third uniform
        ap, xp, v1p = act[pos], x[pos], v1[pos]
        sp, u = u01_open(s[pos])
        st[ap] = sp
        v = v1p * v1p * v1p
        lhs = ln2 * o.log2(u.astype(t))
        rhs = t(0.5) * xp * xp + d - d * v + d * (ln2 * o.log2(v))
        margin[ap] = np.minimum(margin[ap], np.abs(lhs.astype(np.float64) - rhs.astype(np.float64)))
        acc = lhs < rhs
        value[ap[acc]] = (boost[ap] * d * v)[acc]
        keep = np.ones(act.size, bool)
        keep[np.flatnonzero(pos)[acc]] = False
        act = act[keep]
    fell = np.zeros(n, bool)
    fell[act] = True
    return dict(value=value, iters=iters, cont=cont, fell=fell, margin=margin, log2u0=log2u0, r=r_out, x=x_out, v1=v1_out)


def draw_bound(ref):
    """per draw of a float64 `gamma03` result: (A, B) with relative error <= A + sum_f B[f] * E_f, E_f = 2 * ulps_f * U.
    (A draw that fell through has no v term; none does in any test.)"""
    L0 = np.abs(ref["log2u0"].astype(np.float64))
    r, x, v1 = (np.abs(ref[k].astype(np.float64)) for k in ("r", "x", "v1"))
    cx = float(C_MT) * x
    amp = np.where(ref["fell"], 0.0, 3.0 / v1)         # the cube of v1 = 1 + c x: three times its relative error
    kb = np.log(2.0) * L0 / float(ALPHA)
    A = kb * U + amp * (cx * 1.5 * U + cx * U + v1 * U) + 4 * U
    B = dict(log=kb + amp * cx * 0.5, exp=np.ones_like(L0), cos=amp * float(C_MT) * r, sqrt=amp * cx)
    return A, B


def rel_bound(A, B, ulps):
    return A + sum(B[f] * (2.0 * ulps[f] * U) for f in ("log", "exp", "cos", "sqrt"))


def wave_sum_fixed_f32(g):
    """the kernel's sum of one sample's f32 draws g[nc]: lane l adds its children l, l + 64, ... in order, then wave_sum_fixed
    (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror, (row0 + row1) + (row2 + row3)); f32 throughout"""
    lanes = np.zeros(256, np.float32)
    lanes[:g.size] = g
    lanes = lanes.reshape(4, 64)
    v = lanes[0].copy()
    for k in range(1, (g.size + 63) // 64):
        v = v + lanes[k]
    v = v.reshape(4, 2, 2, 2, 2)                       # row, half, pair of quads' halves ... : lane = 16 row + 8 h + 4 q + 2 a + b
    v = v[..., 0] + v[..., 1]
    v = v[..., 0] + v[..., 1]
    v = v[..., 0] + v[..., 1]
    v = v[..., 0] + v[..., 1]
    return F32(F32(v[0] + v[1]) + F32(v[2] + v[3]))


def samples(seed, game_id, root_ply, sim, nc, dtype=np.float64):
    """the root noise of the searches (game_id[k], root_ply[k], sim[k]) (arrays broadcast against each other; scalars allowed) at a root
    of nc children, under the kernel's key sc_rng(seed, game, root_ply, 3, sim * 256 + i).  -> dict: noise [K, nc] (normalised, dtype),
    g [K, nc] (the draws), flagged [K] (some draw's margin < MARGIN), draws (the `gamma03` dict, arrays [K * nc])"""
    game_id, root_ply, sim = np.broadcast_arrays(np.atleast_1d(np.asarray(game_id, np.uint64)),
                                                 np.atleast_1d(np.asarray(root_ply, np.uint64)), np.atleast_1d(np.asarray(sim, np.uint64)))
    K = game_id.size
    i = np.arange(nc, dtype=np.uint64)[None, :]
    ctr = sim.reshape(K, 1) * np.uint64(256) + i
    key = sc_rng(seed, game_id.reshape(K, 1), root_ply.reshape(K, 1), 3, ctr)
    dr = gamma03(key.reshape(-1), dtype)
    g = dr["value"].reshape(K, nc)
    if np.dtype(dtype) == np.float32:
        tot = np.array([wave_sum_fixed_f32(row) for row in g], np.float32)
    else:
        tot = g.sum(axis=1)
    return dict(noise=g / tot[:, None], g=g, flagged=(dr["margin"].reshape(K, nc) < MARGIN).any(axis=1), draws=dr)


def noise(seed, game_id, root_ply, sim, nc, dtype=np.float64):
    """the normalised sample(s) alone: [nc] for scalar arguments, else [K, nc]"""
    out = samples(seed, game_id, root_ply, sim, nc, dtype)["noise"]
    return out[0] if np.ndim(game_id) == 0 and np.ndim(root_ply) == 0 and np.ndim(sim) == 0 else out


def sample_bound(ref, nc):
    """per entry of the float64 `samples` result `ref`: (A, B), |device - ref.noise| <= ref.noise * (A + sum_f B[f] * E_f)"""
    K = ref["noise"].shape[0]
    A, B = draw_bound(ref["draws"])
    w = ref["noise"].astype(np.float64)                # the draws' weights in the sum (they add up to 1)
    depth = (nc + 63) // 64 - 1 + 6
    A = A.reshape(K, nc)
    A = A + (w * A).sum(axis=1, keepdims=True) + depth * U + U
    Bs = {}
    for f, b in B.items():
        b = b.reshape(K, nc)
        Bs[f] = b + (w * b).sum(axis=1, keepdims=True)
    return A, Bs


def min_common_ulps(err, ref_noise, A, B):
    """the smallest e with err <= ref * rel_bound(A, B, all four constants = e) everywhere: what a measurement reports"""
    slope = sum(B.values()) * 2.0 * U
    need = (err / ref_noise - A) / slope
    return float(max(need.max(), 0.0))
