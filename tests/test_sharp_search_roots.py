"""CPU: tests/golden/sharp_search_roots.json (tools/gen_sharp_search_roots.py) is what the live oracle computes, is well formed,
and lies in the regime it was recorded for -- sharp priors, long narrow lines -- so that the GPU test that measures the engine
against it (tests/test_gpu_sharp_search.py) cannot be satisfied by a flat network."""
import json
import os

import numpy as np
import pytest

import gen_sharp_search_roots as gen
import sharp_nets
from support import GOLD


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(GOLD, "sharp_search_roots.json")) as fh:
        return json.load(fh)


def test_fixture_is_well_formed(orc, fx):
    """the configuration and the 48 lines are the generator's; the moves are the oracle's legal moves in its order; every row of
    counts has one entry per move and sums to R - 1"""
    assert fx["config"] == gen.CONFIG and set(fx["kinds"]) == set(sharp_nets.KINDS)
    R = fx["config"]["rollout"]
    lines = gen.fixture_lines()
    assert len(fx["positions"]) == 48 and [p["line"].split() for p in fx["positions"]] == lines
    for p in fx["positions"]:
        st = orc.State()
        for m in p["line"].split():
            st.push(m)
        assert p["moves"].split() == [orc.uci(m) for m in st.legal_moves()]
    for kind, rows in fx["kinds"].items():
        assert len(rows) == 48
        for p, row in zip(fx["positions"], rows):
            for mode in gen.MODES:
                assert len(row[mode]) == len(p["moves"].split()) and sum(row[mode]) == R - 1 and min(row[mode]) >= 0, (kind, mode, p["line"])
            assert 2 <= row["longest_path"] <= R


@pytest.mark.parametrize("kind", list(sharp_nets.KINDS))
def test_fp32_counts_are_the_live_oracles(orc, fx, kind):
    """two positions per kind searched again with the fp32 oracle network: moves, counts and the longest path are the recorded ones
    (the first position, and of the others the one with the longest recorded path)"""
    c = fx["config"]
    net = sharp_nets.oracle_net(orc, c["n_res_blocks"], c["channels"], c["seed"], kind, "fp32")
    rows = fx["kinds"][kind]
    deepest = max(range(1, 48), key=lambda i: rows[i]["longest_path"])
    for i in (0, deepest):
        moves, counts, longest = gen.root_search(net, fx["positions"][i]["line"].split())
        assert moves == fx["positions"][i]["moves"].split()
        assert counts == rows[i]["fp32"] and longest == rows[i]["longest_path"], (kind, i)


def test_fixture_is_in_the_sharp_regime(fx):
    """on the fp32 counts alone: the most visited root child holds at least half of the visits on average (a seed-initialised
    network: 19 %), the longest path of a search averages at least 7 nodes (flat: none longer than 6) and reaches 12 somewhere, for either kind"""
    R = fx["config"]["rollout"]
    for kind, rows in fx["kinds"].items():
        share = np.mean([max(r["fp32"]) / (R - 1) for r in rows])
        paths = [r["longest_path"] for r in rows]
        print(f"{kind}: mean share of the most visited child {share:.3f}, longest path mean {np.mean(paths):.2f}, max {max(paths)}")
        assert share >= 0.5, kind
        assert np.mean(paths) >= 7 and max(paths) >= 12, kind
