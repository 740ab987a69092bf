"""Perft, checks that need no GPU: the Python yardstick of the GPU tests (tests/perft_ref.py) against the table of expected values
and against the oracle's own perft; sc_perft declared, bound and exported; bad arguments refused before anything looks for a
device; without a device the call fails loudly; scamd.rules importable without torch."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import perft_ref
from support import ROOT, _p, scamd_built  # noqa: F401

SMALL_ROWS = [(fen, d) for fen, rows in perft_ref.TABLE.items() for d, row in rows.items() if row[0] <= perft_ref.SMALL]


@pytest.mark.parametrize("fen,depth", SMALL_ROWS, ids=[f"{f.split()[0][:12]}-d{d}" for f, d in SMALL_ROWS])
def test_yardstick_meets_the_table(orc, fen, depth):
    """every row of at most about 10^5 nodes, every column the table has; the divide sums to the nodes and is the oracle's"""
    st = orc.State(fen)
    r = perft_ref.perft(st, depth)
    want = perft_ref.TABLE[fen][depth]
    got = (r["nodes"],) + tuple(r["kinds"])
    assert [g for g, w in zip(got, want) if w is not None] == [w for w in want if w is not None]
    assert r["nodes"] == st.perft(depth) == sum(n for _, n in r["divide"])
    assert r["divide"] == perft_ref.divide_by_oracle(st, depth)
    assert st.fen() == orc.State(fen).fen()   # the walk leaves the state as it found it


def test_table_has_the_probes_it_names(orc):
    """one of Black's six moves in the pawn ending stalemates White, one of White's 24 queen moves mates; the wide position has
    218 moves; mates are counted among the checks; depth 0 is one node"""
    st = orc.State(perft_ref.PAWN_ENDING)
    stale = 0
    for m in st.legal_moves():
        st.push(m)
        stale += int(not st.legal_moves() and not st.is_check())
        st.pop()
    assert stale == 1
    assert perft_ref.perft(orc.State(perft_ref.QUEEN_MATE), 1)["kinds"][4:] == [4, 1]
    assert len(orc.State(perft_ref.WIDE).legal_moves()) == 218 and orc.State(perft_ref.WIDE).perft(3) == 19073
    assert perft_ref.perft(orc.State(), 0) == dict(nodes=1, kinds=[0] * 6, divide=[])
    for fen, rows in perft_ref.TABLE.items():
        for row in rows.values():
            assert row[6] is None or row[6] <= row[5] <= row[0]


# ---------------------------------------------------------------------------------- the ABI
def _declared(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sc_engine.h")).read(), flags=re.S)
    m = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, hdr, flags=re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_symbols_are_declared_bound_and_exported(scamd):
    nm = subprocess.run(["nm", "-D", "--defined-only", scamd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TW"}
    for name, n_par in (("sc_perft", 14), ("sc_perft_last_timing", 2)):
        assert _declared(name) == n_par, name
        assert len(scamd.binding.ABI[name][1]) == n_par, name
        assert name in exported, name
    hdr = open(os.path.join(ROOT, "include", "sc_engine.h")).read()
    for k, name in enumerate(("NODES", "CAPTURES", "EP", "CASTLES", "PROMOTIONS", "CHECKS", "CHECKMATES")):
        assert re.search(r"\bSC_PERFT_%s = %d\b" % (name, k), hdr), name
    from scamd import rules
    assert callable(rules.perft) and callable(rules.legal_moves) and rules.KINDS == perft_ref.KINDS
    assert not hasattr(scamd, "perft") and not hasattr(scamd, "legal_moves")   # the submodule's, not the package's


def _call(L, n=1, depth=1, max_frontier=0, nodes=True, div=(False, False), moves=None, move_off=None):
    out = dict(nodes=np.zeros(max(n, 1), np.uint64), dm=np.zeros((max(n, 1), 224), np.uint16), dn=np.zeros((max(n, 1), 224), np.uint64))
    return L.sc_perft(0, n, None, None, None if moves is None else _p(moves), None if move_off is None else _p(move_off), depth, max_frontier,
                      _p(out["nodes"]) if nodes else None, None, _p(out["dm"]) if div[0] else None, _p(out["dn"]) if div[1] else None, None, None)


def test_bad_arguments_are_refused_before_the_device(scamd):
    L = scamd.lib()
    assert _call(L, n=-1) == -1 and "sc_perft" in L.sc_last_error().decode()
    assert _call(L, n=1 << 24) == -1
    for depth in (-1, 17):
        assert _call(L, depth=depth) == -1 and "depth" in L.sc_last_error().decode()
    for mf in (255, (1 << 24) + 1, 1, -1):
        assert _call(L, max_frontier=mf) == -1 and "max_frontier" in L.sc_last_error().decode()
    assert _call(L, nodes=False) == -1 and "nodes" in L.sc_last_error().decode()
    assert _call(L, div=(True, False)) == -1 and _call(L, div=(False, True)) == -1      # NULL exactly when the other is
    one = np.array([1804], np.uint16)   # e2e4
    assert _call(L, moves=one) == -1                                                    # moves without offsets
    assert _call(L, move_off=np.array([0, 1], np.uint32)) == -1                         # offsets that name moves, and none given
    assert _call(L, moves=one, move_off=np.array([1, 0], np.uint32)) == -1              # not monotonic
    assert _call(L, n=0) == 0 and _call(L, n=0, nodes=True, depth=16, max_frontier=256) == 0   # nothing to do is no error


def test_without_a_device_the_call_fails_loudly(scamd):
    """a valid call: -3 and "no HIP device" where there is none (and 20 nodes where there is one)"""
    L = scamd.lib()
    nodes = np.zeros(1, np.uint64)
    rc = L.sc_perft(0, 1, None, None, None, None, 1, 0, _p(nodes), None, None, None, None, None)
    from scamd import rules
    if L.sc_device_count() > 0:
        assert rc == 0 and nodes[0] == 20
        assert rules.legal_moves([[]])[0][:2] == ["g1h3", "g1f3"]
    else:
        assert rc == -3 and "no HIP device" in L.sc_last_error().decode() and nodes[0] == 0
        with pytest.raises(scamd.EngineError, match="no HIP device"):
            rules.perft([[]], 1)
        with pytest.raises(scamd.EngineError, match="no HIP device"):
            rules.legal_moves([[]], fens=[perft_ref.KIWI])


def test_rules_module_imports_without_torch():
    code = ("import sys; sys.path.insert(0, %r); from scamd import rules; import scamd; "
            "print('torch' in sys.modules, sorted(n for n in ('perft', 'legal_moves') if hasattr(scamd, n)))" % os.path.join(ROOT, "smart-chess-rust_amd"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True)
    assert r.stdout.split(None, 1) == ["False", "[]\n"], r.stdout + r.stderr
