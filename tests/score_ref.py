"""The yardstick of the scoring tests: the reference's judging formulas (scripts/train.py validation_step / training_step's
pi_entropy, scripts/validate_model.py) restated in float64 numpy on log-probabilities and values, and the error bounds the GPU
results are held to.  tests/test_score_abi.py checks this module against torch on the CPU.

Bounds (u = 2^-24, the unit roundoff of float32).  The kernels (score_kernels.hip) document every sum over a row as a fixed tree
13 additions deep, on products that are rounded before they are added (-ffp-contract=off): K = 14 roundings per term.  The
exponential is HIP's expf, which the HIP math-function table lists at 1 ulp: EPS_EXP = 2^-23."""
import numpy as np

U = 2.0 ** -24
K = 14              # 1 product / difference rounding + 13 levels of the summation tree (<= 16, the issue's cap for a tree over 4672)
EPS_EXP = 2.0 ** -23   # expf, 1 ulp (HIP math-function table)
TINY = 2.0 ** -126


def dense_from_sparse(dist_legal, legal_idx, n_legal):
    """zeros(P, 4672) with the shares of the entries i < n_legal added at their action index (the padding is not touched)"""
    P = dist_legal.shape[0]
    out = np.zeros((P, 4672), np.float32)
    keep = np.arange(dist_legal.shape[1])[None, :] < np.asarray(n_legal)[:, None]
    rows = np.repeat(np.arange(P), dist_legal.shape[1]).reshape(P, -1)
    np.add.at(out, (rows[keep], legal_idx.astype(np.int64)[keep]), dist_legal[keep])
    return out


def score(logp, value, dist, outcome):
    """per position, float64: ce = -sum dist * logp over the non-zero shares, se = (value - outcome)^2,
    ent = -sum exp(logp) * logp; and their bounds"""
    lp = logp.astype(np.float64)
    d = dist.astype(np.float64)
    nz = d != 0
    prod = np.where(nz, d * np.where(nz, lp, 0.0), 0.0)
    ce = -prod.sum(1)
    v, o = value.astype(np.float64), outcome.astype(np.float64)
    se = (v - o) ** 2
    p = np.exp(lp)
    ent = -(p * lp).sum(1)
    b_ce = 256 * U * np.abs(prod).sum(1)
    b_ent = (K * U + EPS_EXP + np.abs(lp).max(1) * U) * (p * (1 + np.abs(lp))).sum(1)
    b_se = 4 * U * se + TINY
    return dict(ce=ce, se=se, ent=ent, b_ce=b_ce, b_ent=b_ent, b_se=b_se)


def compare(logp1, value1, logp2, value2):
    """per position, float64: tv = sum |exp(logp1) - exp(logp2)| / 2, dv = |value1 - value2|; and their bounds"""
    l1, l2 = logp1.astype(np.float64), logp2.astype(np.float64)
    p1, p2 = np.exp(l1), np.exp(l2)
    tv = np.abs(p1 - p2).sum(1) / 2
    dv = np.abs(value1.astype(np.float64) - value2.astype(np.float64))
    b_tv = (K * U + EPS_EXP + np.maximum(np.abs(l1).max(1), np.abs(l2).max(1)) * U) * ((p1 + p2) / 2).sum(1)
    b_dv = 4 * U * dv + TINY
    return dict(tv=tv, dv=dv, b_tv=b_tv, b_dv=b_dv)


def mean_bound(x):
    """|device mean - numpy float64 mean| of the float32 values x"""
    x = np.asarray(x, np.float64)
    return x.size * 2.0 ** -53 * np.abs(x).sum()
