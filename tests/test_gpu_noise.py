"""GPU (-m gpu): the root's Dirichlet(0.3) noise as the kernels that ship draw it (`gamma03` and the normalisation in
csrc/search_select.hpp, compiled into k_mcts and into the fused k_step), draw by draw against the float64 replay of tests/noise_ref.py.
Every test goes through `SelfPlay(with_noise=True)`, one simulation per `enqueue(1)`, and `get_noise`: no debug kernel.

What the replay is worth as a reference is shown on the CPU (tests/test_noise_ref.py: the law of the draws, the bound's form).  Here:
  a. every sample of every slot at every simulation >= 1 equals the replay within the per-sample bound, at root widths of every lane round;
  b. the key is (seed, game id, ply, simulation, child) and nothing else: bit-equal samples across slots, handles and recycled slots;
  c. the search stays in lockstep with the oracle when the oracle is handed the device's own noise (the prior mix, the uct words);
  d. the fused one-launch step and the two-launch form draw the same bits.

The bound (noise_ref.sample_bound) counts the roundings of the arithmetic and one constant per hardware function, in ulps
(noise_ref.HW_ULP).  Only finished samples can be read back, so the four constants are measured jointly: the smallest common value at
which every unflagged entry of every sample of a width passes (noise_ref.min_common_ulps, printed by every comparison).  MEASURED on the
MI355X, test (a), per root width 2 / 20 / 63 / 64 / 65 / 82 / 128 / 129 / 137 / 191 / 193 / 218:
0.000 / 0.053 / 0.152 / 0.000 / 0.016 / 0.105 / 0.116 / 0.169 / 0.243 / 0.041 / 0.042 / 0.022 ulps (largest relative error of an entry
1.03e-5, at 218); test (d) 0.014.  COMMITTED: 0.5 ulps for each of the four, twice the largest (the project's convention: bounds = 2x
the maxima observed).  A sample is skipped only where the replay itself flags it (a draw whose accept/reject margin is below 1e-5: 0 to 13
of the 2496 samples of a width), and at most 1 % of the samples of a width may be."""
import numpy as np
import pytest

import noise_ref as nr
from helpers import _same_tree, bits, load_edge_lines
from lines import WIDE, WIDE137, pushed
from support import scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu
MAXC = 224
SENTINEL = -7.25             # what the host writes into the noise buffer before the run: kept past nc
N_SIMS = 40

# Roots of every lane round (a lane draws for children lane, lane + 64, ...; wave_sum_fixed runs over 1..4 registers per lane), on both
# sides of every boundary.  Lines: prefixes of WIDE137 pass through 64, 65, 63 and 128 legal moves.  FENs: the 218-move position (the
# most legal moves any position has: 9 queens, and 16 men whose 8 promotions the 8 missing pawns pay for, so the device's validation
# accepts it) and the same with queens taken off.
F218 = "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1"
FENS = {129: "R6R/8/6Q1/4Q3/8/Q4Q2/pp6/kBNN1KB1 w - - 0 1", 191: "R6R/3Q4/6Q1/4Q3/2Q4Q/5Q2/pp1Q4/kBNN1KB1 w - - 0 1",
        193: "R6R/3Q4/1Q4Q1/8/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1", 218: F218}


def _edge_line(name, plies):
    return next(ln["uci"] for ln in load_edge_lines() if ln["name"] == name)[:plies]


def _root(nc):
    """(moves, fen) of a root with nc legal moves"""
    if nc in FENS:
        return [], FENS[nc]
    if nc == 2:      # a check evasion (tests/golden/edge_lines.json): 3 ... Qh4+ against e4 / f3, two replies
        return _edge_line("king_xray_step_walk0", 4), None
    return {20: [], 64: WIDE137[:38], 65: WIDE137[:56], 63: WIDE137[:78], 82: WIDE, 128: WIDE137[:108], 137: WIDE137}[nc], None


def _assert_equals_replay(dev, seed, games, plies, sims, nc, what, cap=True):
    """dev [K, nc] f32 samples read back from the device against the replay under the keys (games[k], plies[k], sims[k])"""
    dev = np.asarray(dev, np.float32).reshape(-1, nc)
    games, plies, sims = np.broadcast_arrays(np.ravel(games), np.ravel(plies), np.ravel(sims))
    x = dev.astype(np.float64)
    assert np.isfinite(x).all() and (x >= 0).all(), what            # flagged samples included
    assert np.abs(x.sum(axis=1) - 1).max() < 1e-5, what
    ref = nr.samples(seed, games, plies, sims, nc)
    A, B = nr.sample_bound(ref, nc)
    keep = ~ref["flagged"]
    err = np.abs(x - ref["noise"])
    need = nr.min_common_ulps(err[keep], ref["noise"][keep], A[keep], {f: b[keep] for f, b in B.items()})
    rel = (err / ref["noise"])[keep]
    print(f"{what}: {dev.shape[0]} samples of {nc}, flagged {int((~keep).sum())}; unflagged: max relative error {rel.max():.3e}, "
          f"smallest common hardware constant that passes {need:.3f} ulps (committed {nr.HW_ULP})")
    if cap:
        assert (~keep).mean() <= nr.MAX_FLAGGED, what
    bad = (err > ref["noise"] * nr.rel_bound(A, B, nr.HW_ULP)) & keep[:, None]
    for k, i in np.argwhere(bad)[:10]:
        print(f"{what}: game {games[k]} ply {plies[k]} sim {sims[k]} child {i}: device {dev[k, i]!r} "
              f"replay {ref['noise'][k, i]!r} iterations {ref['draws']['iters'].reshape(-1, nc)[k, i]}")
    assert not bad.any(), f"{what}: {int(bad.sum())} entries of {int(bad.any(axis=1).sum())} unflagged samples are outside the bound"
    return need


def _run_fixed_root(sp, n_slots, nc, n_sims):
    """n_sims simulations of one ply, one per launch -> noise [n_sims, n_slots, 224] as read back after each (simulation 0 expands the
    root and draws nothing); checks the slots' counters on the way"""
    out = np.zeros((n_sims, n_slots, MAXC), np.float32)
    for s in range(n_sims):
        sp.enqueue(1)
        sp.sync()
        for g in range(n_slots):
            out[s, g] = sp.get_noise(g, MAXC)
    for g in range(n_slots):
        assert sp.slot(g)["sim"] == n_sims and int(sp.tree(g, cap=1)["n_child"][0]) == nc
    return out


@pytest.mark.parametrize("nc", [2, 20, 63, 64, 65, 82, 128, 129, 137, 191, 193, 218])
def test_every_sample_equals_the_replay(scamd, orc, nc):
    """64 games at a root of nc children, 40 simulations: each of the 64 x 39 samples against noise_ref.noise(seed, game, ply, sim, nc);
    entries >= 0, sum 1; the buffer behind the nc-th entry keeps the host's bytes.  218 children: the position F218 through
    set_position(fen=...), which the device accepts.  Measured figures per width: the module's docstring."""
    from scamd.fen import Positions
    moves, fen = _root(nc)
    st = orc.State(fen) if fen else pushed(orc, moves)
    assert len(st.legal_moves()) == nc and st.outcome() is None
    seed, first = 8, (0 if nc == 20 else 1000 + nc)
    sp = scamd.SelfPlay(None, n_slots=64, n_games=64, rollout_num=400, num_steps=4, evaluator="synth", with_noise=True, seed=seed,
                        first_game_id=first)
    pos = Positions([fen]).check(for_search=True) if fen else None
    for g in range(64):
        if moves or fen:
            sp.set_position(g, moves, fen=(pos, 0) if fen else None)
        sp.set_noise(g, np.full(MAXC, SENTINEL, np.float32))
    ply = len(moves)
    assert all(sp.slot(g)["ply"] == ply and sp.slot(g)["game_id"] == first + g for g in (0, 63))
    got = _run_fixed_root(sp, 64, nc, N_SIMS)
    assert (got[0] == SENTINEL).all()                       # simulation 0: the root has no children yet
    assert (got[1:, :, nc:] == SENTINEL).all()              # never a store behind the root's children
    sims, games = np.meshgrid(np.arange(1, N_SIMS), first + np.arange(64), indexing="ij")
    _assert_equals_replay(got[1:, :, :nc], seed, games.ravel(), ply, sims.ravel(), nc, f"root of {nc}")
    assert sp.stats()["error_flags"] == 0
    sp.close()
    if pos is not None:
        pos.close()


def test_a_single_reply_draws_nothing(scamd, orc):
    """a root with ONE child takes no arg-max and draws no noise: the buffer keeps the host's bytes"""
    line = _edge_line("ep_evades_pawn_check_walk1", 5)
    assert len(pushed(orc, line).legal_moves()) == 1
    sp = scamd.SelfPlay(None, n_slots=2, n_games=2, rollout_num=400, num_steps=4, evaluator="synth", with_noise=True, seed=8)
    sp.set_position(1, line)
    sp.set_noise(1, np.full(MAXC, SENTINEL, np.float32))
    sp.enqueue(6)
    assert (sp.get_noise(1, MAXC) == SENTINEL).all() and sp.slot(1)["sim"] == 6
    sp.close()


# ---------------------------------------------------------------------------------- b. the key
GAME_CFG = dict(rollout_num=6, num_steps=3, cpuct=2.5, temperature=1.0, temperature_switch=100, with_noise=True, outcome_gate=100,
                evaluator="synth", seed=21)


def _record(sp, n_slots, n_steps):
    """whole games, one simulation per launch -> {(game id, ply, simulation): (slot, nc, noise [nc])} for every search that drew noise"""
    out = {}
    for _ in range(n_steps):
        pre = []
        for g in range(n_slots):
            s = sp.slot(g)
            drew = s["status"] == 1 and s["sim"] >= 1          # ST_ACTIVE, root expanded
            pre.append((s, int(sp.tree(g, cap=1)["n_child"][0]) if drew else 0))
        sp.enqueue(1)
        sp.sync()
        for g, (s, nc) in enumerate(pre):
            if nc > 1:
                key = (s["game_id"], s["ply"], s["sim"])
                assert key not in out, key
                out[key] = (g, nc, sp.get_noise(g, nc).copy())
    return out


def _assert_same_bits(a, b, keys, what):
    assert keys
    for k in keys:
        assert k in a and k in b, (what, k)
        assert a[k][1] == b[k][1] and np.array_equal(bits(a[k][2]), bits(b[k][2])), (what, k, a[k][0], b[k][0])


def test_key_is_seed_game_ply_simulation_child(scamd):
    """the same game draws the same bits wherever it runs: on slot g of a 64-slot handle, on a recycled slot of an 8-slot handle
    (n_games > n_slots), under first_game_id = 100 against a handle that counts from 0, at ply > 0, and in a game that set_position starts
    at ply 2; different games, plies and simulations draw different samples; every sample equals the replay under that key"""
    keys_of = lambda games: [(g, p, s) for g in games for p in range(3) for s in range(1, 6)]   # noqa: E731
    # Y: ids 0 .. 109 on 64 slots: games 64 .. 109 run on recycled slots
    y = scamd.SelfPlay(None, n_slots=64, n_games=110, **GAME_CFG)
    Y = _record(y, 64, 40)
    assert y.stats()["games_finished"] == 110 and y.stats()["error_flags"] == 0
    assert set(Y) == set(keys_of(range(110)))
    assert all(Y[(g, 0, 1)][0] == g for g in range(64))
    # X: ids 0 .. 23 on 8 slots, three games per slot
    x = scamd.SelfPlay(None, n_slots=8, n_games=24, **GAME_CFG)
    X = _record(x, 8, 60)
    assert x.stats()["games_finished"] == 24 and set(X) == set(keys_of(range(24)))
    assert all(X[(g, 0, 1)][0] < 8 for g in range(24))
    _assert_same_bits(X, Y, keys_of(range(24)), "8 slots against 64")
    # Z: first_game_id = 100 on 8 slots: slot j plays game 100 + j, which Y played on a recycled slot
    z = scamd.SelfPlay(None, n_slots=8, n_games=8, first_game_id=100, **GAME_CFG)
    Z = _record(z, 8, 20)
    assert set(Z) == set(keys_of(range(100, 108))) and all(Z[(100 + j, 0, 1)][0] == j for j in range(8))
    _assert_same_bits(Z, Y, keys_of(range(100, 108)), "first_game_id 100 against ids from 0")
    # W: game 10 started by set_position at ply 2 from the moves Y's game 10 played
    line = [st[0] for st in y.trace(10)["steps"][:2]]
    w = scamd.SelfPlay(None, n_slots=2, n_games=2, first_game_id=10, **GAME_CFG)
    w.set_position(0, line)
    assert w.slot(0)["ply"] == 2 and w.slot(0)["game_id"] == 10
    Wr = _record(w, 1, 6)
    assert set(Wr) == {(10, 2, s) for s in range(1, 6)}
    _assert_same_bits(Wr, Y, sorted(Wr), "set_position at ply 2")
    # anything else in the key changes the sample
    assert len({tuple(bits(v[2]).tolist()) for v in Y.values()}) == len(Y)
    firsts = {}
    for (g, p, s), v in Y.items():
        firsts.setdefault((p, s), set()).add(int(bits(v[2])[0]))
    assert all(len(f) == 110 for f in firsts.values())       # child 0 alone tells the 110 games apart at every (ply, simulation)
    # ... and the key is the replay's: every sample of Y, by root width
    by_nc = {}
    for k, v in Y.items():
        by_nc.setdefault(v[1], []).append(k)
    assert len(by_nc) > 3
    for nc, keys in sorted(by_nc.items()):
        g, p, s = (np.array(c) for c in zip(*keys))
        _assert_equals_replay(np.stack([Y[k][2] for k in keys]), GAME_CFG["seed"], g, p, s, nc, f"games, roots of {nc}", cap=False)
    for h in (x, y, z, w):
        h.close()


# ---------------------------------------------------------------------------------- c. lockstep on the device's own noise
@pytest.mark.parametrize("line,n_root,R", [([], 20, 120), (["e2e4", "c7c5", "g1f3"], None, 120), (["f2f3", "e7e5", "g2g4"], None, 120),
                                           (WIDE, 82, 180), (WIDE137, 137, 180)], ids=["start20", "sicilian", "grob", "wide82", "wide137"])
def test_search_lockstep_exact_on_device_noise(scamd, orc, line, n_root, R):
    """test_search_lockstep_exact / test_search_wide_root_lockstep_exact with external_noise=False: after every simulation the noise the
    device drew is read back and handed to the oracle's simulation; node pools, uct words and paths stay identical -- the
    `prior * (1 - epsilon) + noise * epsilon` mix and the uct words of the path that draws on the device"""
    sp = scamd.SelfPlay(None, n_slots=2, n_games=2, rollout_num=R, num_steps=140, cpuct=2.5, with_noise=True, epsilon=0.15,
                        evaluator="synth", external_noise=False, seed=3)
    st = pushed(orc, line)
    nc = len(st.legal_moves())
    assert n_root in (None, nc)
    sp.set_position(1, line)
    srch = orc.Search(st)
    seen = set()
    for s in range(R - 1):
        sp.enqueue(1)
        nz = sp.get_noise(1, nc).copy()
        if s >= 1:
            assert abs(float(nz.astype(np.float64).sum()) - 1) < 1e-5
            seen.add(nz.tobytes())
        srch.sim(cpuct=2.5, epsilon=0.15, with_noise=True, noise=nz.astype(np.float64))
        assert list(sp.slot(1)["path"]) == list(srch.last_path()), s
        if s % 7 == 0 or s > R - 5:
            assert _same_tree(sp.tree(1), srch.dump()), s
    assert len(seen) == R - 2                                  # fresh noise at every simulation
    kids = sp.tree(1)["n"][1:1 + nc]
    assert sp.tree(1)["n_child"][0] == nc and (nc <= 64 or (kids[:64].sum() > 0 and kids[64:].sum() > 0))
    assert sp.stats()["error_flags"] == 0
    sp.close()


# ---------------------------------------------------------------------------------- d. both builds
def test_fused_step_and_two_launch_form_draw_the_same_bits(scamd):
    """`gamma03` is compiled twice, into k_mcts (contraction off) and into the fused k_step (contraction on in the unit): with a 1 x 128
    network on 64 slots, the one-launch form and the two-launch form (enable_timing(1)) leave bit-identical noise in every slot after each
    of 20 simulations, and both equal the replay"""
    eng = scamd.Engine(1, 128, seed=5, precision="bf16")
    cfg = dict(n_slots=64, n_games=64, rollout_num=400, num_steps=4, cpuct=2.5, with_noise=True, seed=8, first_game_id=7)
    got = []
    for timed in (False, True):
        sp = scamd.SelfPlay(eng, **cfg)
        if timed:
            sp.enable_timing(1)
        else:
            assert sp.launches_per_step() == 1
        got.append(_run_fixed_root(sp, 64, 20, 21))
        if timed:
            assert sp.timing(reset=False)["tower_launches"] >= 20
        assert sp.stats()["error_flags"] == 0
        sp.close()
    assert np.array_equal(bits(got[0]), bits(got[1]))
    sims, games = np.meshgrid(np.arange(1, 21), 7 + np.arange(64), indexing="ij")
    for form, a in zip(("one launch", "two launches"), got):
        _assert_equals_replay(a[1:, :, :20], 8, games.ravel(), 0, sims.ravel(), 20, form)
    eng.close()
