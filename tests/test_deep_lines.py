"""The preconditions of tests/test_gpu_deep_paths.py, asserted with the oracle alone (no GPU): the positions of
tests/deep_lines.py give the trees that file says they give -- forced chains, paths far longer than 64 and 128 nodes, a tree of
two nodes -- so that the device tests cannot go shallow unnoticed."""
import numpy as np
import pytest

import deep_lines as dl


@pytest.mark.parametrize("name", dl.FORCED)
def test_forced_has_one_reply_at_every_ply(orc, name):
    st = orc.State(dl.POSITIONS[name])
    seen = []
    for ply in range(300):
        lm = st.legal_moves()
        assert len(lm) == 1, (ply, st.fen())
        seen.append(st.fen().split()[0])
        st.push(lm[0])
    assert seen[:4] == seen[4:8] and len(set(seen)) == 4          # period 4: kings out, kings back


@pytest.mark.parametrize("name", dl.FORCED)
def test_forced_search_is_a_chain(orc, name):
    """simulation s walks the whole chain: its path has s nodes; afterwards the tree is a chain of s + 1 nodes with n[i] = s - i"""
    srch = orc.Search(orc.State(dl.POSITIONS[name]))
    values = []
    for s in range(1, 401):
        srch.sim(cpuct=2.5, with_noise=False)
        assert list(srch.last_path()) == list(range(s)), s
        if s <= 260:
            values.append(srch.dump()["q"][s - 1])                 # the leaf's first backup: its own value
    d = srch.dump()
    assert len(d["n"]) == 401
    assert np.array_equal(d["n"], 400 - np.arange(401)) and np.array_equal(d["n_child"][:400], np.ones(400, np.int32))
    assert np.array_equal(d["first_child"][:400], 1 + np.arange(400)) and d["n_child"][400] == 0
    assert len({np.float32(v).tobytes() for v in values}) == 260   # a value backed up into the wrong level changes a sum


@pytest.mark.parametrize("evaluator", list(dl.EVALUATORS))
@pytest.mark.parametrize("name", dl.COMB)
def test_comb_paths_run_past_one_and_two_wavefronts(orc, name, evaluator):
    srch, lens = dl.path_lengths(orc, dl.POSITIONS[name], evaluator, 260)
    d = srch.dump()
    over64, over128 = sum(n > 64 for n in lens), sum(n > 128 for n in lens)
    jumps = sum(a > 64 and b < a - 8 for a, b in zip(lens, lens[1:]))       # a long path followed by a clearly shorter one
    print(f"{name} {evaluator}: longest path {max(lens)}, {over64} over 64, {over128} over 128, {int((d['n_child'] == 2).sum())} two-child nodes, "
          f"{jumps} long-then-shorter pairs")
    f64, f128 = dl.COMB_FLOORS[evaluator]
    assert over64 >= f64 and over128 >= f128
    assert d["n_child"].max() == 2 and (d["n_child"] == 2).sum() >= 2 and (d["n_child"] == 1).sum() > 64
    assert jumps >= 2           # the stale-prefetch case: path[] still holds the longer path's tail when the shorter one is backed up
    assert d["n"][0] == 260


def test_comb_reaches_almost_300_levels_at_400_simulations(orc):
    for name in dl.COMB:
        _, lens = dl.path_lengths(orc, dl.POSITIONS[name], "synth", 400)
        print(f"{name} synth, 400 simulations: longest path {max(lens)}")
        assert max(lens) > 256                                     # level 192 and beyond: a fourth round of lanes in the backup


def test_sink_tree_has_two_nodes(orc):
    st = orc.State(dl.SINK)
    lm = st.legal_moves()
    assert [orc.uci(m) for m in lm] == ["h1g1"]
    st.push(lm[0])
    assert st.legal_moves() == [] and not st.is_check() and st.outcome()["termination"] == "Stalemate"
    for evaluator in dl.EVALUATORS:
        srch, lens = dl.path_lengths(orc, dl.SINK, evaluator, 260)
        d = srch.dump()
        assert len(d["n"]) == 2 and d["n"][0] == 260 and d["n"][1] == 259 and lens == [1] + [2] * 259
