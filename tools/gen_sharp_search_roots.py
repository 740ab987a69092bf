"""Writes tests/golden/sharp_search_roots.json: the root visit counts of the CPU oracle's search with sharp-prior networks
(tests/sharp_nets.py: g4v2, g8) on the 48 fixture positions of the statistical search test -- the yardstick of
tests/test_gpu_sharp_search.py, recorded once because the fp32 oracle network needs about 1.2 s per 96-simulation search at
6 x 128 and a GPU test cannot afford 96 of them.

Configuration: 6 blocks x 128 channels, seed 5, cpuct 2.5, no noise, 96 simulations (the root's children share 95 visits).
Positions: random_games(orc, 70, 60, seed=31), those that are not over, the first 48.  For each kind and position: the root
visit counts with the fp32 oracle network (the yardstick), with its bf16- and fp8-emulating modes (the same quantisation points
as the engine, independent of the engine's code: the expected size of the deviation), and the longest path of the fp32 search
in nodes.  The line and the root's moves (the oracle's legal moves, in its order) are recorded once per position.

CPU only, deterministic; the searches of the 2 x 3 networks run in processes of their own:

    python tools/gen_sharp_search_roots.py [--out tests/golden/sharp_search_roots.json] [--jobs 6]
"""
import argparse
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from oracle import oracle_py as orc  # noqa: E402
import helpers as H  # noqa: E402
import sharp_nets  # noqa: E402

CONFIG = {"n_res_blocks": 6, "channels": 128, "seed": 5, "cpuct": 2.5, "with_noise": False, "rollout": 96, "positions": 48,
          "games": [70, 60, 31]}
MODES = ("fp32", "bf16", "fp8")


def fixture_lines():
    """the 48 lines of tests/test_gpu_netloop.py's statistical test, as UCI"""
    n, maxlen, seed = CONFIG["games"]
    lines = [[orc.uci(m) for m in g[0]] for g in H.random_games(orc, n, maxlen, seed=seed) if g[1].legal_moves() and g[1].outcome() is None]
    assert len(lines) >= CONFIG["positions"]
    return lines[:CONFIG["positions"]]


def root_search(net, line):
    """(root moves as UCI, root visit counts, longest path in nodes) of CONFIG's search from `line` with the oracle network `net`"""
    st = orc.State()
    for m in line:
        st.push(m)
    srch = orc.Search(st)
    longest = 0
    for _ in range(CONFIG["rollout"]):
        srch.sim(evaluator="orc_eval_net", user=net.h, cpuct=CONFIG["cpuct"], with_noise=CONFIG["with_noise"])
        longest = max(longest, len(srch.last_path()))
    d = srch.dump()
    fc, nc = int(d["first_child"][0]), int(d["n_child"][0])
    return [orc.uci(int(m)) for m in d["move"][fc:fc + nc]], [int(x) for x in d["n"][fc:fc + nc]], longest


def _job(arg):
    kind, mode = arg
    net = sharp_nets.oracle_net(orc, CONFIG["n_res_blocks"], CONFIG["channels"], CONFIG["seed"], kind, mode)
    return kind, mode, [root_search(net, ln) for ln in fixture_lines()]


def generate(jobs):
    orc.build()
    lines = fixture_lines()
    args = [(k, m) for k in sharp_nets.KINDS for m in MODES]
    if jobs > 1:
        with multiprocessing.Pool(min(jobs, len(args))) as pool:
            got = pool.map(_job, args)
    else:
        got = [_job(a) for a in args]
    res = {(k, m): r for k, m, r in got}
    moves = [r[0] for r in res[next(iter(sharp_nets.KINDS)), "fp32"]]
    assert all([r[0] for r in rows] == moves for rows in res.values())
    out = ['{"config": ' + json.dumps(CONFIG, sort_keys=True) + ",", ' "positions": [']
    out += ["  " + json.dumps({"line": " ".join(ln), "moves": " ".join(mv)}, sort_keys=True) + ("," if i + 1 < len(lines) else "")
            for i, (ln, mv) in enumerate(zip(lines, moves))]
    out += [" ],", ' "kinds": {']
    for j, kind in enumerate(sharp_nets.KINDS):
        out.append(f'  "{kind}": [')
        for i in range(len(lines)):
            row = {m: res[kind, m][i][1] for m in MODES}
            row["longest_path"] = res[kind, "fp32"][i][2]
            out.append("   " + json.dumps(row, sort_keys=True, separators=(",", ":")) + ("," if i + 1 < len(lines) else ""))
        out.append("  ]" + ("," if j + 1 < len(sharp_nets.KINDS) else ""))
    out += [" }", "}"]
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "sharp_search_roots.json"))
    ap.add_argument("--jobs", type=int, default=6)
    a = ap.parse_args()
    text = generate(a.jobs)
    json.loads(text)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(f"wrote {a.out}: {len(text)} bytes")
