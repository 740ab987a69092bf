"""Inputs and a plain restatement for the tests of the end-of-ply move choice (mcts::step, src/mcts.rs:298-317, and
NNPlayer::bestmove, src/play.rs:268-277).

The weighted branch turns a libm result into a discrete decision: `WeightedIndex` over `(n as f32).powf(1 / temp)`, sequential
f32 cumulative sums, `index = #{i < n - 1 : cum[i] <= u * total}`.  Rust's `f32::powf` is the host libm's `powf`, so that
function -- called through ctypes, never numpy's own f32 power -- is the reference for a single weight.  A one-ulp difference
in one weight moves one cumulative boundary by an ulp, which only a `u` right next to that boundary can see: `bracket_us`
makes those."""
import ctypes
import random

import numpy as np

F = np.float32
LATTICE = 1 << 24            # the kernels draw u = k / 2^24, k = the top 24 bits of the counter RNG
U_LAST = F(1.0) - F(2.0 ** -24)
TEMPS = [0.1, 0.25, 0.3, 0.5, 0.6, 0.75, 0.9, 1.25, 1.5, 2.0, 3.0, 10.0]
NCS = [1, 2, 20, 63, 64, 65, 128, 129, 223, 224]
ROLLOUTS = [2, 20, 180, 800]
SHAPES = ["zeros", "near_equal", "all_equal", "dominant", "tail"]
MAX_MOVES = 224

_libm = ctypes.CDLL("libm.so.6")
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]


def host_powf(x, y):
    """the host libm's powf on f32 arguments, as f32"""
    return F(_libm.powf(float(F(x)), float(F(y))))


def weights_ref(n_act, temp):
    """(f32 cumulative sums, f32 total) of the weights at temp != 0, summed in index order like WeightedIndex::new"""
    power = F(1.0) / F(temp)
    total, cum = F(0.0), []
    with np.errstate(all="ignore"):
        for v in n_act:
            total = F(total + host_powf(F(int(v)), power))
            cum.append(total)
    return cum, total


def choose_ref(n_act, temp, u, tie_random=False):
    """(choice, total): mcts::step; with tie_random the temperature-0 rule of play.rs:268-277 (k = floor(u * count)-th
    most-visited child in index order, the build-defined draw)"""
    n_act = [int(v) for v in n_act]
    if F(temp) == F(0.0):
        mx = max(n_act)
        idx = [i for i, v in enumerate(n_act) if v == mx]
        if not tie_random:
            return idx[0], F(0.0)
        k = int(F(F(u) * F(len(idx))))
        return idx[min(k, len(idx) - 1)], F(0.0)
    cum, total = weights_ref(n_act, temp)
    with np.errstate(all="ignore"):
        x = F(F(u) * total)
        return sum(1 for c in cum[:-1] if c <= x), total


def lattice_u(k):
    return F(min(max(int(k), 0), LATTICE - 1)) / F(LATTICE)


def bracket_us(cum, total, boundaries):
    """for each boundary i the lattice points k / 2^24 around cum[i] / total (two on either side)"""
    us = []
    if not np.isfinite(total) or total <= 0:
        return us
    for i in boundaries:
        k0 = int(np.floor(float(cum[i]) / float(total) * LATTICE))
        us += [lattice_u(k0 + d) for d in (-1, 0, 1, 2)]
    return us


def count_vector(shape, nc, total, rnd):
    """nc visit counts; every shape but `all_equal` sums to `total` (= rollouts - 1: the first simulation expands the root)"""
    n = [0] * nc

    def spread(where, amount):
        for _ in range(amount):
            n[rnd.choice(where)] += 1

    if shape == "zeros":                       # few visited children, child 0 unvisited (cum[0] = 0 = x at u = 0)
        free = list(range(1, nc)) or [0]
        spread(rnd.sample(free, max(1, len(free) // 8)), total)
    elif shape == "near_equal":
        for i in range(nc):
            n[i] = total // nc + (i < total % nc)
    elif shape == "all_equal":
        n = [max(1, total // nc)] * nc
    elif shape == "dominant":
        big = rnd.randrange(nc)
        rest = total // 10 if nc > 1 else 0
        n[big] = total - rest
        spread([i for i in range(nc) if i != big] or [big], rest)
    elif shape == "tail":                      # a few heavy children, then a long tail of single visits
        tail = min(max(nc - 3, 0), total // 2)
        for i in range(nc - tail, nc):
            n[i] = 1
        spread(list(range(min(3, nc))), total - tail)
    else:
        raise ValueError(shape)
    assert len(n) == nc and (shape == "all_equal" or sum(n) == total)
    return n


def boundary_cases(seed=1, per_vector_temps=2, n_random_u=3, n_boundaries=6, ncs=NCS):
    """[(n_act, temp, u)]: every nc x rollout x shape, temperatures cycling through TEMPS + [1.0], and for each vector u = 0,
    1 - 2^-24, uniform lattice draws and the lattice points around some cumulative boundaries (the first, the last, the first
    that is not zero, random ones)"""
    rnd = random.Random(seed)
    temps = TEMPS + [1.0]
    cases, t = [], 0
    for nc in ncs:
        for R in ROLLOUTS:
            for shape in SHAPES:
                n = count_vector(shape, nc, R - 1, rnd)
                for _ in range(per_vector_temps):
                    temp = temps[t % len(temps)]
                    t += 1
                    cum, total = weights_ref(n, temp)
                    nz = [i for i in range(nc) if cum[i] > 0]
                    b = {0, max(nc - 2, 0), nc - 1, nz[0] if nz else 0}
                    b |= {rnd.randrange(nc) for _ in range(n_boundaries - len(b))}
                    us = [F(0.0), U_LAST] + [lattice_u(rnd.randrange(LATTICE)) for _ in range(n_random_u)]
                    us += bracket_us(cum, total, sorted(b))
                    seen = set()
                    for u in us:
                        if float(u) not in seen:
                            seen.add(float(u))
                            cases.append((n, temp, u))
    return cases


def degenerate_cases():
    """[(n_act, temp, u)] whose total is 0 or infinite: the reference panics in WeightedIndex::new (AllWeightsZero /
    InvalidWeight), oracle and device quietly return an index"""
    cases = []
    for nc in (1, 2, 20, 65, 224):
        for temp in (1.0, 0.5, 2.0):                    # all counts zero: a rollout budget of 1 expands the root only
            for u in (F(0.0), F(0.5), U_LAST):
                cases.append(([0] * nc, temp, u))
    for n in ([800], [800, 3], [3, 800, 0, 5], [0, 0, 800], [799] + [1] * 223, [1] * 64 + [800] + [0] * 100):
        for temp in (0.05, 0.06):                       # 800^20, 800^(1/0.06) overflow f32
            for u in (F(0.0), F(0.25), U_LAST):
                cases.append((n, temp, u))
    return cases


def pack(cases):
    """(n_act [n][224] i32, nc [n] i32, temperature [n] f32, u [n] f32) of [(n_act, temp, u)]"""
    m = len(cases)
    n_act = np.zeros((m, MAX_MOVES), np.int32)
    nc = np.zeros(m, np.int32)
    temp = np.zeros(m, np.float32)
    u = np.zeros(m, np.float32)
    for i, (n, t, uu) in enumerate(cases):
        n_act[i, :len(n)] = n
        nc[i], temp[i], u[i] = len(n), t, uu
    return n_act, nc, temp, u


def oracle_choices(orc, n_act, nc, temp, u):
    """(choice [n] i32, total [n] f32) from orc_choose_child_total, case by case"""
    L = orc.lib()
    m = len(nc)
    choice = np.zeros(m, np.int32)
    total = np.zeros(m, np.float32)
    t = ctypes.c_float()
    for i in range(m):
        choice[i] = L.orc_choose_child_total(n_act[i].ctypes.data, int(nc[i]), float(temp[i]), float(u[i]), ctypes.byref(t))
        total[i] = t.value
    return choice, total
