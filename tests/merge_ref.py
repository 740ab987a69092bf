"""The yardstick of the merge tests: what sc_merge_positions computes, restated in numpy.  Positions are partitioned by the Python
bytes of (boards, meta, n_legal, legal_idx[:n_legal]); the head of a group is its smallest position, groups are numbered by
ascending head; sums are a loop of np.float32 additions in ascending position, then / np.float32(m).  Every formula is exact: the
GPU results are compared bit for bit."""
import numpy as np

MAX_LEGAL = 218
N_LEGAL = (0, 1, 63, 64, 65, 128, 129, 192, 193, 218)   # the boundaries of the lanes' entries i, i + 64, i + 128, i + 192
KEYS = ("boards", "meta", "dist_legal", "legal_idx", "n_legal", "outcome")


def sample_bytes(src, r):
    """what makes row r a sample of its own; None for n_legal outside 0..218 (the same as nothing)"""
    n = int(src["n_legal"][r])
    if n < 0 or n > MAX_LEGAL:
        return None
    return (src["boards"][r].tobytes(), src["meta"][r].tobytes(), n, src["legal_idx"][r, :n].tobytes())


def partition(src, rows=None, n_in=None):
    """-> group_of int32 [n_in] (-1: row outside the source), groups [[positions ascending]] by ascending head, n_bad"""
    n_src = src["boards"].shape[0]
    rows = np.arange(n_src if n_in is None else n_in) if rows is None else np.asarray(rows)
    group_of = np.full(len(rows), -1, np.int32)
    groups, seen, n_bad = [], {}, 0
    for p, r in enumerate(int(x) for x in rows):
        if r < 0 or r >= n_src:
            n_bad += 1
            continue
        key = sample_bytes(src, r)
        if key is None:
            n_bad += 1
            key = ("alone", p)
        if key not in seen:
            seen[key] = len(groups)
            groups.append([])
        group_of[p] = seen[key]
        groups[seen[key]].append(p)
    return group_of, groups, n_bad


def mean_f32(values):
    """s = x_1; s = s + x_k in float32; s / float32(m)"""
    s = np.float32(values[0])
    for x in values[1:]:
        s = np.float32(s + np.float32(x))
    return np.float32(s / np.float32(len(values)))


def merged_rows(src, groups, rows=None):
    """the merged tensors of a partition (the yardstick's own or the device's): a dict of the six keys plus count and first"""
    n_src = src["boards"].shape[0]
    rows = np.arange(n_src) if rows is None else np.asarray(rows)
    G = len(groups)
    out = dict(boards=np.zeros((G, 8, 8, 112), np.int8), meta=np.zeros((G, 7), np.int32), dist_legal=np.zeros((G, 224), np.float32),
               legal_idx=np.zeros((G, 224), np.uint16), n_legal=np.zeros(G, np.int32), outcome=np.zeros(G, np.float32),
               count=np.zeros(G, np.int32), first=np.zeros(G, np.int32))
    for j, members in enumerate(groups):
        rr = [int(rows[p]) for p in members]
        h, m = rr[0], len(rr)
        for k in KEYS:
            out[k][j] = src[k][h]
        out["count"][j], out["first"][j] = m, members[0]
        if m > 1:
            n = int(src["n_legal"][h])
            with np.errstate(all="ignore"):
                for i in range(n):
                    out["dist_legal"][j, i] = mean_f32([src["dist_legal"][r, i] for r in rr])
                out["outcome"][j] = mean_f32([src["outcome"][r] for r in rr])
    return out


def merge(src, rows=None, n_in=None):
    """-> (merged dict, group_of, counts [groups, bad, key clashes = 0, largest m])"""
    group_of, groups, n_bad = partition(src, rows, n_in)
    out = merged_rows(src, groups, rows)
    return out, group_of, np.array([len(groups), n_bad, 0, max((len(g) for g in groups), default=0)], np.int32)


def make_source(n_src=37, seed=1):
    """distinct rows: random int8 planes (negatives, -128 and 127), meta, n_legal over N_LEGAL, shares inside n_legal 0 or in
    [2^-20, 1] (never subnormal or NaN), outcomes in {-1, 0, 1}; past n_legal NaN shares and action indices up to 65535"""
    rng = np.random.default_rng(seed)
    b = rng.integers(-128, 128, (n_src, 8, 8, 112)).astype(np.int8)
    b[0, 0, 0, :4] = [-128, 127, -1, 1]
    m = rng.integers(-5, 400, (n_src, 7)).astype(np.int32)
    nl = np.array([N_LEGAL[i % len(N_LEGAL)] for i in range(n_src)], np.int32)
    li = np.zeros((n_src, 224), np.uint16)
    for r in range(n_src):
        li[r, :nl[r]] = rng.choice(4672, int(nl[r]), replace=False)
    src = dict(boards=b, meta=m, legal_idx=li, n_legal=nl, dist_legal=np.zeros((n_src, 224), np.float32), outcome=np.zeros(n_src, np.float32))
    fresh_targets(src, rng)
    assert (b < 0).any()
    return src


def fresh_targets(src, rng, rows=None):
    """new shares, outcome and padding garbage for the given rows (all by default), in place: the sample input stays"""
    for r in range(src["boards"].shape[0]) if rows is None else rows:
        n = int(src["n_legal"][r])
        n = n if 0 <= n <= MAX_LEGAL else 0
        sh = (np.float32(2.0) ** -rng.uniform(0, 20, n)).astype(np.float32)
        sh[rng.random(n) < 0.2] = 0.0
        src["dist_legal"][r, :n] = sh
        pad = rng.standard_normal(224 - n).astype(np.float32) * np.float32(1e30)
        pad[rng.random(224 - n) < 0.5] = np.nan
        src["dist_legal"][r, n:] = pad
        src["legal_idx"][r, n:] = rng.integers(0, 65536, 224 - n)
        src["outcome"][r] = rng.integers(-1, 2)
    assert not np.isnan(src["outcome"]).any()


def expand(base, copies, seed=2):
    """copies[r] copies of row r of base, in shuffled order, each with targets and padding of its own -> (source, origin row of
    each position)"""
    rng = np.random.default_rng(seed)
    origin = rng.permutation(np.repeat(np.arange(len(copies)), copies))
    src = {k: np.ascontiguousarray(base[k][origin]) for k in KEYS}
    fresh_targets(src, rng)
    return src, origin
