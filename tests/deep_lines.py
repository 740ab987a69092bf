"""Positions whose search trees grow deeper than one 64-lane wavefront: locked pawn endings in which almost every move is forced.

Every per-level structure of the device search is laid out one entry per lane, so level 64 and beyond take a second code
path: the backup's `d = lane + 64` loop behind the 64 prefetched path nodes (search_expand.hpp dev_expand), `s_ps[depth]` and
`path[depth]` in both kernels, the helper wave's DevChain reads of the step kernel, nodes with a single child (the PUCT block
is skipped) and the depth limit.  From positions with many replies a search of a few hundred simulations stays 8 to 20 levels
deep; from these it does not.  tests/test_deep_lines.py holds the oracle to what is said here, tests/test_gpu_deep_paths.py
compares the device with it.

Out of scope: a repetition scan that runs past 64 entries INSIDE the tree part of the chain.  It needs more than 64 forced,
reversible, non-repeating plies, and no such position is known: here the positions repeat with period 4, so a scan meets its
second match (and stops) in its first round of lanes."""

# FORCED: every pawn and both bishops are immobile; each king has one square to go to and one to come back from
# (h1-g1, a8-b8).  Exactly one legal move at every ply: a search of s simulations is a chain of s + 1 nodes.
_FORCED = "k2b4/p1pPp3/P1P1P3/8/8/3p1p1p/3PpP1P/4B2K %s - - 0 1"
# COMB: FORCED plus a white pawn on b2 and a black one on b4.  Either side may spend its one pawn move (b2b3 / b4b3), which is
# irreversible and lands in the middle of a path; the rest is forced.  A short spine of two-child nodes with long forced teeth:
# consecutive simulations follow paths of very different lengths.
_COMB = "k2b4/p1pPp3/P1P1P3/8/1p6/3p1p1p/1P1PpP1P/4B2K %s - - 0 1"
# SINK: White's only move, h1g1, stalemates Black.  Simulation 1 evaluates the root, simulation 2 finds the terminal, every later
# one returns the cached terminal at depth 1: no child list anywhere along the way but the root's single child.
SINK = "k7/Pp6/1P6/8/8/3p1p1p/3PpP1P/4B2K w - - 0 1"

FORCED_W, FORCED_B = _FORCED % "w", _FORCED % "b"
COMB_W, COMB_B = _COMB % "w", _COMB % "b"

POSITIONS = {"forced_w": FORCED_W, "forced_b": FORCED_B, "comb_w": COMB_W, "comb_b": COMB_B, "sink": SINK}
FORCED = ("forced_w", "forced_b")
COMB = ("comb_w", "comb_b")

EVALUATORS = {"synth": "orc_eval_synth", "synth_coarse": "orc_eval_synth_coarse", "synth_uniform": "orc_eval_synth_uniform"}

# COMB, 260 simulations, cpuct 2.5, no noise: floors under what the oracle measures (tests/test_deep_lines.py prints the figures):
# evaluator -> (simulations whose path is longer than 64 nodes, ... longer than 128)
COMB_FLOORS = {"synth": (100, 30), "synth_coarse": (60, 0), "synth_uniform": (60, 0)}


def path_lengths(orc, fen, evaluator, sims, cpuct=2.5):
    """(the oracle's search after `sims` simulations from `fen`, the length of every simulation's path)"""
    srch = orc.Search(orc.State(fen))
    lens = []
    for _ in range(sims):
        srch.sim(evaluator=EVALUATORS[evaluator], cpuct=cpuct, with_noise=False)
        lens.append(len(srch.last_path()))
    return srch, lens
