"""The yardstick of the minibatch tests: what sc_gather_batch computes for sample b from row r = rows[b] of the compact tensors,
restated in numpy -- the reference's _prepare (py/dataset.py:31-44), the mirrored outcome (:61-62), Board::rotate()'s meta
and the dense visit shares.  Every formula is exact: the GPU results are compared bit for bit, there is no tolerance."""
import numpy as np

ROW = 4672
MAX_LEGAL = 218


def boards(src_boards, r):
    """float32 [112][8][8] = (float) int8 [8][8][112], planes first"""
    return src_boards[r].astype(np.float32).transpose(2, 0, 1)


def meta(src_meta, r, mirror):
    """float32 [7]; mirrored: with t = m[0], [1 - t, m[1] + (t == 1), m[4], m[5], m[2], m[3], m[6]]"""
    m = src_meta[r].astype(np.int64)
    if mirror:
        t = m[0]
        m = np.array([1 - t, m[1] + (1 if t == 1 else 0), m[4], m[5], m[2], m[3], m[6]], np.int64)
    return m.astype(np.int32).astype(np.float32)


def dist(dist_legal, legal_idx, n_legal, r):
    """float32 [4672]: zeros, dist_legal[r][i] at legal_idx[r][i] for i < n_legal[r] only; all NaN for n_legal outside 0..218 or
    an action index >= 4672 among those entries"""
    n = int(n_legal[r])
    out = np.zeros(ROW, np.float32)
    if n < 0 or n > MAX_LEGAL or (legal_idx[r, :n].astype(np.int64) >= ROW).any():
        out[:] = np.nan
        return out
    out[legal_idx[r, :n].astype(np.int64)] = dist_legal[r, :n]
    return out


def outcome(src_outcome, r, mirror):
    return np.float32(-src_outcome[r]) if mirror else np.float32(src_outcome[r])


def gather(src, rows, mirror=None):
    """-> boards [B,112,8,8], meta [B,7], dist [B,4672], outcome [B], n_bad; a row outside the source: all NaN"""
    B, n_src = len(rows), src["boards"].shape[0]
    ob, om = np.zeros((B, 112, 8, 8), np.float32), np.zeros((B, 7), np.float32)
    od, oo = np.zeros((B, ROW), np.float32), np.zeros(B, np.float32)
    n_bad = 0
    for b, r in enumerate(int(x) for x in rows):
        mir = mirror is not None and mirror[b] != 0
        if r < 0 or r >= n_src:
            ob[b], om[b], od[b], oo[b] = np.nan, np.nan, np.nan, np.nan
            n_bad += 1
            continue
        ob[b] = boards(src["boards"], r)
        om[b] = meta(src["meta"], r, mir)
        od[b] = dist(src["dist_legal"], src["legal_idx"], src["n_legal"], r)
        oo[b] = outcome(src["outcome"], r, mir)
        n_bad += int(np.isnan(od[b, 0]))
    return ob, om, od, oo, n_bad
