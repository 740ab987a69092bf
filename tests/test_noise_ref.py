"""CPU tests of the root-noise yardstick (tests/noise_ref.py): its key function equals the engine's and the oracle's, its draws have the
Gamma(0.3, 1) law the Dirichlet(0.3) noise is built from (src/mcts.rs:123-130), the rare paths of Marsaglia-Tsang occur and are counted,
and the per-draw error bound holds between the float32 and the float64 replay.  The GPU tests (tests/test_gpu_noise.py) then only have to
show that the kernels equal the replay."""
import numpy as np
import pytest

import noise_ref as nr
from support import rules_host  # noqa: F401

N_DRAWS = 2_000_000
KEY = dict(seed=8, game=5, ply=0)


def test_key_function_equals_engine_and_oracle(H, orc):
    """sc_rng of the replay == sct_rng (csrc/chess_rules.hpp on the host) == orc_rng (the oracle's own) on a few hundred tuples"""
    L = orc.lib()
    rnd = np.random.RandomState(7)
    tuples = [(0, 0, 0, 1, 0), (123, 7, 33, 3, 99), (2 ** 63, 5, 1, 2, 0), (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1, 3, 2 ** 48 - 1),
              (8, 5, 0, 3, 40 * 256 + 217)]
    def word(max_bits):     # a random word of a random length: small ids and counters as well as full 64-bit seeds
        return int.from_bytes(rnd.bytes(8), "little") >> int(rnd.randint(64 - max_bits, 64))

    for _ in range(300):
        tuples.append((word(64), word(64), word(10), int(rnd.randint(0, 4)), word(48)))
    arr = np.array(tuples, np.uint64)
    got = nr.sc_rng(*(arr[:, k] for k in range(5)))
    for t, v in zip(tuples, got):
        want = H.sct_rng(*t)
        assert int(v) == want == L.orc_rng(*t), t
        assert int(nr.sc_rng(*t)) == want, t      # scalar arguments too
    assert len(set(got.tolist())) == len(set(tuples))


@pytest.fixture(scope="module")
def draws():
    """2 000 000 draws under one key, counters 0 .. 2e6 - 1: the float64 yardstick and the float32 replay of the same streams"""
    st = nr.sc_rng(KEY["seed"], KEY["game"], KEY["ply"], 3, np.arange(N_DRAWS, dtype=np.uint64))
    return nr.gamma03(st, np.float64), nr.gamma03(st, np.float32)


def test_draws_have_the_gamma_law(draws):
    """Kolmogorov-Smirnov against Gamma(0.3, 1) (CDF: torch.special.gammainc in float64), mean, variance, lag-1 correlation"""
    import torch
    x = draws[0]["value"]
    n = x.size
    xs = np.sort(x)
    cdf = torch.special.gammainc(torch.full((n,), 0.3, dtype=torch.float64), torch.from_numpy(xs)).numpy()
    i = np.arange(1, n + 1, dtype=np.float64)
    D = max((i / n - cdf).max(), (cdf - (i - 1) / n).max())
    mean, var = x.mean(), x.var()
    r1 = np.corrcoef(x[:-1], x[1:])[0, 1]
    print(f"KS D*sqrt(n) = {D * np.sqrt(n):.3f}  mean {mean:.5f}  var {var:.5f}  lag-1 r*sqrt(n) = {r1 * np.sqrt(n):.3f}")
    assert D * np.sqrt(n) < 1.95                   # the 0.001 critical value
    assert abs(mean / 0.3 - 1) < 0.01 and abs(var / 0.3 - 1) < 0.01
    assert abs(r1) * np.sqrt(n) < 4
    assert (x > 0).all() and np.isfinite(x).all()


def test_rare_paths_occur_and_are_counted(draws):
    """more than one iteration, the `v <= 0` continue (which draws no third uniform), and never the 64-iteration fall-through"""
    ref = draws[0]
    multi = int((ref["iters"] > 1).sum())
    cont = int((ref["cont"] > 0).sum())
    print(f"more than one iteration: {multi} ({100.0 * multi / N_DRAWS:.2f} %)  took the v <= 0 continue: {cont}  "
          f"largest iteration count: {ref['iters'].max()}")
    assert 0.02 * N_DRAWS < multi < 0.05 * N_DRAWS  # Marsaglia-Tsang at shape 1.3 rejects about one candidate in thirty
    assert cont > 0
    assert ref["iters"].max() < nr.MAX_ITER and not ref["fell"].any()
    # the stream position after a `continue` differs from that after a rejection: both kinds of second iteration are present
    second = ref["iters"] > 1
    assert (second & (ref["cont"] == 0)).any() and (second & (ref["cont"] == ref["iters"] - 1)).any()


def test_float32_replay_within_the_bound_of_the_float64_replay(draws):
    """no accept/reject decision differs between the two replays among draws whose margin is >= 1e-5, and every such draw of the
    float32 replay (correctly rounded functions: half an ulp each) is within the per-draw bound -- the bound's form, before any GPU
    value is compared with it"""
    ref, f32 = draws
    clear = ref["margin"] >= nr.MARGIN
    differ = (ref["iters"] != f32["iters"]) | (ref["cont"] != f32["cont"])
    print(f"draws with margin < {nr.MARGIN}: {int((~clear).sum())}; decisions that differ: {int(differ.sum())}, "
          f"among clear draws: {int((differ & clear).sum())}")
    assert not (differ & clear).any()
    A, B = nr.draw_bound(ref)
    bound = nr.rel_bound(A, B, nr.HALF_ULP)
    v64 = ref["value"]
    rel = np.abs(f32["value"].astype(np.float64) - v64) / v64
    ok = clear & ~differ
    print(f"float32 vs float64: max relative difference {rel[ok].max():.3e}, 99.99th percentile {np.percentile(rel[ok], 99.99):.3e}, "
          f"largest share of its bound {(rel[ok] / bound[ok]).max():.3f}")
    assert (rel[clear] <= bound[clear]).all()
    # the bound is no blanket: at the typical draw it is a few tens of roundings (the exponent of the boost, |log2 u0| ln 2 / 0.3 of
    # them, leads), and the worst float32 draw uses more than half of its bound
    assert np.median(bound) < 32 * nr.U and (rel[ok] / bound[ok]).max() > 0.5


def test_normalised_sample_and_flagged_share():
    """`noise` sums to 1 at every root width, the float32 sample (fixed-order sum) stays within the per-sample bound, and the keys the GPU
    tests use flag less than the cap at the widest root"""
    for nc in (2, 20, 64, 65, 137, 218):
        ref = nr.samples(8, np.arange(64)[:, None], 0, np.arange(1, 41)[None, :], nc)
        f32 = nr.samples(8, np.arange(64)[:, None], 0, np.arange(1, 41)[None, :], nc, np.float32)
        assert ref["noise"].shape == (2560, nc) and np.abs(ref["noise"].sum(axis=1) - 1).max() < 1e-12
        assert np.abs(f32["noise"].astype(np.float64).sum(axis=1) - 1).max() < 1e-5 and (f32["noise"] >= 0).all()
        share = ref["flagged"].mean()
        print(f"width {nc}: flagged {100 * share:.2f} % of 2560 samples")
        assert share <= nr.MAX_FLAGGED
        A, B = nr.sample_bound(ref, nc)
        keep = ~ref["flagged"]
        err = np.abs(f32["noise"].astype(np.float64) - ref["noise"])
        assert (err[keep] <= (ref["noise"] * nr.rel_bound(A, B, nr.HALF_ULP))[keep]).all()
    assert np.array_equal(nr.noise(8, 5, 0, 7, 20), nr.samples(8, [5], [0], [7], 20)["noise"][0])
