"""GPU (-m gpu): the fp8 (OCP e4m3) tower of BASELINE configs[4] -- v_mfma_scale_f32_32x32x64_f8f6f4 convs with per-output-
channel power-of-two weight scales -- through the C ABI.  There is no reference counterpart, so the
tolerance is the build's stated one: against the fp32 vectors produced by the reference module, prior total variation < 0.05
and |value| error < 0.05; and the root's most visited move of a search agrees with the bf16 engine's on >= 90 % of the
fixture searches.  Against the oracle's fp8-emulating mode (same quantisation rules) the first layers agree to fp32
round-off; deeper, single e4m3 rounding flips (a 6 % step) make the two drift apart, so those bounds are statistical."""
import os

import numpy as np
import pytest

from helpers import random_games
from support import GOLD, scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu


def _tv(a, b):
    return 0.5 * np.abs(np.exp(a.astype(np.float64)) - np.exp(b.astype(np.float64))).sum(axis=-1)


@pytest.mark.parametrize("C", [128, 256])
def test_fp8_first_layers_equal_the_emulating_oracle(scamd, orc, C):
    """stem (e4m3 weights with their channel scales in the MFMA block scales, exact 0/1 inputs) and the first residual
    block: the fp32 residual stream equals the oracle's fp8-emulating mode to round-off -- operand lane maps, scale bytes,
    clamp and rounding of the activations are all the oracle's"""
    g = np.load(os.path.join(GOLD, "nn_ref_b1_c256.npz"))
    eng = scamd.Engine(1, C, seed=9, precision="fp8")
    assert eng.precision == "fp8"
    net0, net1 = orc.Net(0, C, seed=9, emulate_fp8=True), orc.Net(1, C, seed=9, emulate_fp8=True)
    for k in range(3):
        stem = eng.debug(g["boards"][k:k + 1], g["meta"][k:k + 1], 0)[0]
        lat = eng.debug(g["boards"][k:k + 1], g["meta"][k:k + 1], 1000)[0]
        o0 = net0.forward(g["boards"][k], g["meta"][k], latent=True)[2]     # (the first tensors of a deeper net are the same)
        o1 = net1.forward(g["boards"][k], g["meta"][k], latent=True)[2]
        print(f"C={C} k={k}: stem max|d|={np.abs(stem - o0).max():.2e} block1 max|d|={np.abs(lat - o1).max():.2e} (max|x| {np.abs(o1).max():.2f})")
        assert np.abs(stem - o0).max() < 2e-4
        # one rounding flip of a conv input moves a few outputs by ~1e-2: allow a handful, not a systematic error
        d = np.abs(lat - o1)
        assert np.median(d) < 1e-4 and (d > 0.05).mean() < 0.01
    eng.close()


@pytest.mark.parametrize("C,nb", [(128, 3), (256, 2), (128, 10), (256, 10)])
def test_fp8_network_vs_fp8_emulating_oracle(scamd, orc, C, nb):
    g = np.load(os.path.join(GOLD, "nn_ref_b1_c256.npz"))
    eng = scamd.Engine(nb, C, seed=9, precision="fp8")
    net = orc.Net(nb, C, seed=9, emulate_fp8=True)
    logp, val = eng.forward(g["boards"][:4], g["meta"][:4])
    assert np.isfinite(logp).all() and np.abs(np.exp(logp.astype(np.float64)).sum(axis=1) - 1).max() < 1e-4
    dl, dv, tv = [], [], []
    for k in range(4):
        ol, ov = net.forward(g["boards"][k], g["meta"][k])
        dl.append(np.abs(logp[k] - ol).max())
        dv.append(abs(val[k] - ov))
        tv.append(_tv(logp[k], ol))
    print(f"fp8 {nb}x{C} vs fp8 oracle: max|dlogp|={max(dl):.4f} max|dvalue|={max(dv):.5f} max TVD={max(tv):.5f}")
    assert max(dl) < 0.7 and max(dv) < 0.035 and max(tv) < 0.05
    eng.close()


@pytest.mark.parametrize("nb", [1, 10, 19, 20])
def test_fp8_within_stated_tolerance_of_reference_goldens(scamd, orc, nb):
    """the claim: vs the fp32 vectors of the reference module, total variation of the policy < 0.05 and |value| error < 0.05
    -- over all 4672 actions and over the renormalised legal-move priors the search consumes (Game::predict contract)"""
    g = np.load(os.path.join(GOLD, f"nn_ref_b{nb}_c256.npz"))
    eng = scamd.Engine(nb, 256, seed=int(g["seed"]), precision="fp8")
    logp, val = eng.forward(g["boards"], g["meta"])
    tv = _tv(logp, g["logp"])
    print(f"fp8 {nb}x256 vs reference: max|dlogp|={np.abs(logp - g['logp']).max():.4f} max|dvalue|={np.abs(val - g['value']).max():.4f} max TVD={tv.max():.4f}")
    assert tv.max() < 0.05 and np.abs(val - g["value"]).max() < 0.05
    # batch independence / determinism in fp8 too
    l2, v2 = eng.forward(g["boards"][::-1], g["meta"][::-1])
    assert np.array_equal(l2[::-1], logp) and np.array_equal(v2[::-1], val)
    # legal-move priors of the start position through the predict contract
    hip = scamd.ChessHip(eng)
    steps, pri, v = hip.predict([])
    st = orc.State()
    e = np.exp(g["logp"][0][[orc.move_index(m, st.turn) for m in st.legal_moves()]].astype(np.float64))
    assert steps == st.legal_moves() and 0.5 * np.abs(pri - e / (e.sum() + 1e-5)).sum() < 0.05 and abs(v - g["value"][0]) < 0.05
    eng.close()


def test_fp8_10x128_within_stated_tolerance_of_reference_blocks(scamd):
    """BASELINE configs[4]'s network at the width the fp8 bench lines use (10 x 128): the same claim against the vectors of the
    128-wide network assembled from the reference's ResBlockSE / ValueHead classes (tools/gen_golden_nn.py)"""
    g = np.load(os.path.join(GOLD, "nn_ref_b10_c128.npz"))
    eng = scamd.Engine(10, 128, seed=int(g["seed"]), precision="fp8")
    logp, val = eng.forward(g["boards"], g["meta"])
    tv = _tv(logp, g["logp"])
    print(f"fp8 10x128 vs reference blocks: max|dlogp|={np.abs(logp - g['logp']).max():.4f} max|dvalue|={np.abs(val - g['value']).max():.4f} max TVD={tv.max():.4f}")
    assert tv.max() < 0.05 and np.abs(val - g["value"]).max() < 0.05
    eng.close()


def test_fp8_export_blob_equals_quantise_at_load(scamd, tmp_path):
    """three routes to the same fp8 engine, bit-identical outputs: the SCW2 export (tools/scw.py: e4m3 bytes + channel
    exponents), an fp32 SCW1 blob quantised at load (sc_net_config.precision), and the seeded init quantised at load"""
    import scw
    sd = scw.prng_state_dict(2, 128, 42)
    p1, p2 = str(tmp_path / "w.scw"), str(tmp_path / "w8.scw")
    scw.write_scw(p1, sd, 2, 128)
    scw.write_scw(p2, sd, 2, 128, fp8=True)
    g = np.load(os.path.join(GOLD, "nn_ref_b1_c256.npz"))
    outs = []
    for kw in (dict(n_res_blocks=2, channels=128, seed=42, precision="fp8"), dict(weights=p1, precision="fp8"), dict(weights=p2)):
        e = scamd.Engine(**kw)
        assert e.precision == "fp8"
        outs.append(e.forward(g["boards"][:3], g["meta"][:3]))
        e.close()
    for l, v in outs[1:]:
        assert np.array_equal(l, outs[0][0]) and np.array_equal(v, outs[0][1])
    bf = scamd.Engine(weights=p1)
    assert bf.precision == "bf16" and not np.array_equal(bf.forward(g["boards"][:3], g["meta"][:3])[0], outs[0][0])
    bf.close()


def test_fp8_search_agrees_with_bf16(scamd, orc):
    """equal root arg-max-visit move between the bf16 and the fp8 engine on the fixture searches (SURVEY.md appendix B:
    >= 90 %); same search code, same seeds, only the network precision differs"""
    lines = [[orc.uci(m) for m in g[0]] for g in random_games(orc, 70, 60, seed=31) if g[1].legal_moves() and g[1].outcome() is None][:48]
    nb, C, R = 6, 128, 96
    a, b = scamd.Engine(nb, C, seed=5), scamd.Engine(nb, C, seed=5, precision="fp8")
    same = tot = 0
    for ln in lines:
        ra = scamd.search(a, ln, R, cpuct=2.5)[1]
        rb = scamd.search(b, ln, R, cpuct=2.5)[1]
        assert [c[0] for c in ra] == [c[0] for c in rb] and sum(c[1] for c in rb) == R - 1
        best_a = max(ra, key=lambda c: c[1])
        nb_ = dict((c[0], c[1]) for c in rb)
        top_b = max(nb_.values())
        same += nb_[best_a[0]] == top_b          # bf16's most visited move is (one of) fp8's most visited
        tot += 1
    print(f"fp8 vs bf16 root arg-max-visit agreement: {same}/{tot}")
    assert tot >= 40 and same / tot >= 0.9
    a.close()
    b.close()


def test_fp8_selfplay_is_deterministic_and_legal(scamd, orc):
    eng = scamd.Engine(2, 128, seed=3, precision="fp8")
    runs = []
    for _ in range(2):
        sp = scamd.SelfPlay(eng, n_slots=16, n_games=16, rollout_num=24, num_steps=8, with_noise=True, seed=9)
        sp.run()
        assert sp.stats()["error_flags"] == 0
        runs.append([sp.trace(g) for g in range(16)])
        sp.close()
    assert runs[0] == runs[1]
    for t in runs[0][:4]:
        st = orc.State()
        for mv, q, kids in t["steps"]:
            assert [k[0] for k in kids] == st.legal_uci() and sum(k[1] for k in kids) == 23
            st.push(mv)
    eng.close()


@pytest.mark.parametrize("slots,games,R", [(1, 2, 5), (300, 340, 4), (513, 513, 3)])
def test_fp8_selfplay_edge_configurations(scamd, slots, games, R):
    """one slot; more slots than CUs (the narrow fp8 tower runs two fused workgroups per CU up to 512 slots); more than
    that (separate launches): every game finishes, every ply's visits add up"""
    eng = scamd.Engine(2, 128, seed=1, precision="fp8")
    sp = scamd.SelfPlay(eng, n_slots=slots, n_games=games, rollout_num=R, num_steps=3, temperature=0.0, temperature_switch=1, with_noise=True,
                        seed=3, outcome_gate=0)
    sp.run()
    st = sp.stats()
    assert st["games_finished"] == games and st["error_flags"] == 0 and st["games_active"] == 0
    for g in range(0, games, 7):
        t = sp.trace(g)
        assert t is not None and 1 <= len(t["steps"]) <= 3 and all(sum(c[1] for c in s[2]) == R - 1 for s in t["steps"])
    sp.close()
    eng.close()


def test_corrupt_fp8_blobs_are_rejected_at_load(scamd, tmp_path):
    """a channel exponent outside the exporter's [-100, 100] (127 + e is the E8M0 scale byte: -128 wraps to the
    NaN code, 127 to 2^127), an e4m3 NaN code, or an e4m3 tensor in a blob whose header says bf16 must fail the load --
    not produce an engine whose activations are NaN or inf"""
    import struct
    import scw
    sd = scw.prng_state_dict(1, 128, 3)
    good = str(tmp_path / "good8.scw")
    scw.write_scw(good, sd, 1, 128, fp8=True)
    blob = bytearray(open(good, "rb").read())
    # first tensor of the table is the stem conv (e4m3): header 20 B, tensor header 28 B + enc 4 B, then its exponents
    assert struct.unpack("<I", blob[20 + 28:20 + 32])[0] == 1
    e0 = 20 + 32
    n_out = struct.unpack("<I", blob[20 + 4:20 + 8])[0]
    scamd.Engine(weights=good).close()
    for name, patch in (("exp_minus128", (e0, 0x80)), ("exp_plus127", (e0 + 5, 0x7F)), ("exp_101", (e0 + 1, 101)),
                        ("nan_code", (e0 + n_out + 17, 0x7F)), ("neg_nan_code", (e0 + n_out + 18, 0xFF)), ("header_says_bf16", (16, 0))):
        bad = bytearray(blob)
        bad[patch[0]] = patch[1]
        p = str(tmp_path / f"{name}.scw")
        open(p, "wb").write(bytes(bad))
        with pytest.raises(scamd.EngineError, match="bad fp8 tensor"):
            scamd.Engine(weights=p)
    ok = bytearray(blob)
    ok[e0] = 0x9C   # -100: the edge of the range still loads
    p = str(tmp_path / "edge.scw")
    open(p, "wb").write(bytes(ok))
    scamd.Engine(weights=p).close()
