"""Networks with sharp priors, for the tests that put one inside the search: plain data and three constructors, no test.

A seed-initialised network has nearly flat priors (6 x 128, seed 5, 96 simulations on the 48 fixture positions: the most visited
root child gets 19 % of the visits, no path is longer than 6 nodes); a trained one is sharp.  The two recipes the project already
uses to get a trained network's output range out of the build-owned init, under one name each:
  g4v2   policy_head.model.3.weight x 4 and value_head.ffn.2.weight x 2: tests/golden/nn_ref_b10_c256_sharp.npz (tools/gen_golden_nn.py)
  g8     policy_head.model.3.weight x 8, nothing else: bench.py's sharp_prior_engine (the `also_sharp_priors` line)
The scaled tensors are the same fp32 numbers for the oracle (set_tensor) and for the engine (a weight blob)."""
import numpy as np

import scw

KINDS = {
    "g4v2": {"policy_head.model.3.weight": 4.0, "value_head.ffn.2.weight": 2.0},
    "g8": {"policy_head.model.3.weight": 8.0},
}
MODES = {"fp32": {}, "bf16": {"emulate_bf16": True}, "fp8": {"emulate_fp8": True}}   # the oracle network's arithmetic


def state_dict(nb, C, seed, kind):
    """scw.prng_state_dict with the tensors of KINDS[kind] scaled (in fp32, as the golden's generator and bench.py do)"""
    sd = scw.prng_state_dict(nb, C, seed)
    for name, gain in KINDS[kind].items():
        sd[name] = sd[name] * np.float32(gain)
    return sd


def oracle_net(orc, nb, C, seed, kind, mode="fp32"):
    """orc.Net on the same weights; mode: fp32, or the emulation of the engine's bf16 / fp8 operand rounding (oracle/nn.c)"""
    net = orc.Net(nb, C, seed=seed, **MODES[mode])
    sd = state_dict(nb, C, seed, kind)
    for i, (name, _, _, _) in enumerate(scw.tensor_table(nb, C)):
        if name in KINDS[kind]:
            net.set_tensor(i, sd[name])
    return net


def engine(scamd, tmp_path, nb, C, seed, kind, precision):
    """scamd.Engine on the same weights, loaded from a blob under tmp_path"""
    path = str(tmp_path / f"sharp_{kind}_{nb}x{C}_s{seed}.scw")
    scw.write_scw(path, state_dict(nb, C, seed, kind), nb, C)
    eng = scamd.Engine(n_res_blocks=nb, channels=C, weights=path, precision=precision)   # the blob decides; the attributes follow these
    assert eng.precision == precision
    return eng
