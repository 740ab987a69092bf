"""CPU: the helpers the test files share (tests/helpers.py, tests/support.py, tests/lines.py), and the rule that keeps them
shared -- nothing imports a test module.

The digests of random_steps were recorded from the copies the test files held before there was one (`_random_steps` of
test_gpu_parity.py for zero_share 0, of test_gpu_score.py for 0.2), so they pin the inputs of every test that draws its steps
from it: the same moves, children and counts, and the same number of calls on the generator."""
import ast
import glob
import hashlib
import os
import random

import numpy as np
import pytest

from helpers import bits, random_games, random_steps
from support import FILL, ROOT, untouched

# (zero_share, seed) -> (SHA-256 of repr(steps), the generator's next draw afterwards)
STEPS = {
    (0.0, 3): ("b57fd9034b32cd569e41066cf2c9253a8e646685320a6dab1541e9c4ea7bb3fe", 0.2952170279346811),
    (0.0, 11): ("85ea4df200d61f3ea857f01120d768f8c0d539941799f9e4ab0a5897837b190b", 0.6873046979546804),
    (0.0, 77): ("8dbb483a9ab5904d5996dbdd104372f93fe7a3b7f4dccff32df4e344b2024dcd", 0.7320036453595985),
    (0.2, 3): ("22cd9fa8c6233ee72f1f8d1b6ae166621093f54275b48fe428fa6c916732247a", 0.7434385974818519),
    (0.2, 11): ("67ac63a90becdcaa2e53823e9b7d49da5b8548b2cfe00354d154da2fce0a014c", 0.21149716445690547),
    (0.2, 77): ("5c34f023f267bb2d9f0bd68e13b56da3fccf5ce94bc8f4f41ad365eea6bf212e", 0.9279882901758504),
}


@pytest.mark.parametrize("zero_share,seed", list(STEPS))
def test_random_steps_draws_what_the_copies_drew(orc, zero_share, seed):
    rnd = random.Random(seed)
    games = [g for g, _ in random_games(orc, 6, 60, seed=seed) if g]
    steps = [random_steps(orc, g, rnd, zero_share) for g in games]
    assert sum(len(g) for g in games) > 50 and all(len(ch) >= 1 for st in steps for _, ch in st)
    zeros = sum(n == 0 for st in steps for _, ch in st for _, n in ch) / sum(len(ch) for st in steps for _, ch in st)
    assert zeros < 0.02 if zero_share == 0 else 0.15 < zeros < 0.25
    assert (hashlib.sha256(repr(steps).encode()).hexdigest(), rnd.random()) == STEPS[zero_share, seed]


def test_bits_is_a_view_of_the_float32_patterns():
    a = np.array([0.0, -0.0, np.nan, 1.0], np.float32)
    b = bits(a)
    assert b.dtype == np.uint32 and b.tolist()[:2] == [0, 0x80000000] and b[3] == 0x3F800000
    assert b[0] != b[1] and a[0] == a[1]          # -0.0 is not +0.0 here
    assert b[2] == bits(a.copy())[2] and a[2] != a[2]   # a NaN maps to itself
    quiet, payload = np.array([0x7FC00000, 0x7FC00001], np.uint32).view(np.float32)
    assert bits(quiet) != bits(payload)


def test_untouched_sees_one_flipped_byte():
    a = np.frombuffer(bytes([FILL]) * 64, np.float32).copy()
    assert FILL == 0x5a and untouched(a) and untouched(a.view(np.int32)) and untouched(a[:0])
    a.view(np.uint8)[37] ^= 1
    assert not untouched(a) and untouched(a[:9]) and untouched(a[10:])


def test_nothing_imports_a_test_module():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py")))
    assert len(files) > 60
    bad = []
    for path in files:
        for node in ast.walk(ast.parse(open(path).read(), path)):
            names = [a.name for a in node.names] if isinstance(node, (ast.Import, ast.ImportFrom)) else []
            names += [node.module or ""] if isinstance(node, ast.ImportFrom) else []
            bad += [(os.path.relpath(path, ROOT), n) for n in names if any(part.startswith("test_") for part in n.split("."))]
    assert not bad, bad
