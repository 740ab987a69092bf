"""The rate tools (tools/*_rate.py on tools/ratelib.py) print what they printed before they shared their loops: each of the seven
tools whose size can be set runs once on a 2 x 128 network as a child process, and its lines are compared with
tests/golden/rate_tool_lines.json -- lines of the tools as they stood one commit before ratelib, each case run twice on one MI355X:

    for run in run1 run2; do for each case below: python tools/<tool>.py <arguments> > $run/<tool>.out; done
    python tests/test_gpu_rate_tools.py run1 run2 > tests/golden/rate_tool_lines.json

Per tool and line the file holds the key tree and the pinned values: the fields whose values agreed between the two runs and
that are not timings by their name (TIMING: a rounded timing can agree by chance), host and date aside -- games, plies, byte
counts, workspace size, groups, duplicate share, word counts, flags.  The rest is measured: timings, rates, ratios of timings, and
sums taken with atomics.  perft_rate (119 M nodes per call) and match_time (whole matches) have no small form; their use of the
shared pieces is covered by tests/test_ratelib.py."""
import json
import math
import os
import re
import subprocess
import sys

import pytest

from support import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "rate_tool_lines.json")
NET = ["--blocks", "2", "--channels", "128"]
CASES = {
    "encode_device_rate": ["--reps", "1"] + NET,
    "san_rate": ["--reps", "1"] + NET,
    "san_write_rate": ["--reps", "1"] + NET,
    "score_rate": ["--reps", "2"] + NET + ["--no-host-route"],
    "merge_rate": ["--reps", "1", "--iters", "1"] + NET,
    "train_batch_rate": ["--reps", "1", "--iters", "1", "--batches", "64"] + NET,
    "fen_rate": ["--positions", "64", "--reps", "1"],
}
# a field that is a time, a rate or a ratio of times, by its name; hbm_bound_ms is computed from the sizes
TIMING = re.compile(r"(^|_)ms($|_)|_per_s$|^x_|_GBps$|^hbm_frac$|_over_")
# never pinned: the machine and the day, what a comparison of two timings decides, and a difference to sums whose order is not fixed
UNPINNED = ("host", "date", "bound", "no_slower_than_torch_route", "max_abs_diff_to_torch_means")


def is_timing(key):
    return key != "hbm_bound_ms" and bool(TIMING.search(key))


def key_tree(v):
    """the keys of a line in their nesting; a list is a leaf"""
    return {k: key_tree(x) for k, x in v.items()} if isinstance(v, dict) else None


def leaves(v, path=()):
    """(path, value) of every leaf of a line"""
    if isinstance(v, dict):
        for k, x in v.items():
            yield from leaves(x, path + (k,))
    else:
        yield path, v


def make_golden(run1, run2):
    gold = {}
    for tool in CASES:
        a, b = ([json.loads(ln) for ln in open(os.path.join(d, tool + ".out"))] for d in (run1, run2))
        assert [key_tree(x) for x in a] == [key_tree(x) for x in b], tool
        gold[tool] = [{"tree": key_tree(x), "pinned": {"/".join(p): v for (p, v), (_, w) in zip(leaves(x), leaves(y))
                                                       if v == w and p[-1] not in UNPINNED and not is_timing(p[-1])}}
                      for x, y in zip(a, b)]
    return gold


def check_timings(d):
    """every timing of a line is finite and positive (a spread: not negative), and min <= median <= max where all three stand"""
    for k, v in d.items():
        if isinstance(v, dict):
            check_timings(v)
        elif is_timing(k):
            xs = v if isinstance(v, list) else [v]
            assert all(isinstance(x, (int, float)) and math.isfinite(x) and (x >= 0 if "spread" in k else x > 0) for x in xs), (k, v)
            if isinstance(v, list) and len(v) == 3:   # [median, min, max]
                assert v[1] <= v[0] <= v[2], (k, v)
            if k + "_min" in d and k + "_max" in d:
                assert d[k + "_min"] <= v <= d[k + "_max"], (k, v, d[k + "_min"], d[k + "_max"])
        else:
            assert not isinstance(v, float) or math.isfinite(v), (k, v)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("tool", list(CASES))
def test_rate_tool_prints_what_the_parent_printed(tool, golden, tmp_path):
    out = tmp_path / "lines.jsonl"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool + ".py")] + CASES[tool] + ["--out", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines()]
    print(r.stdout)
    want = golden[tool]
    assert [key_tree(x) for x in lines] == [w["tree"] for w in want]
    for x, w in zip(lines, want):
        got = {"/".join(p): v for p, v in leaves(x)}
        assert {k: got[k] for k in w["pinned"]} == w["pinned"]
        check_timings(x)
    assert out.read_text() == r.stdout   # the file holds what was printed


if __name__ == "__main__":
    print("{\n" + ",\n".join(f" {json.dumps(t)}: {json.dumps(v)}" for t, v in make_golden(sys.argv[1], sys.argv[2]).items()) + "\n}")
