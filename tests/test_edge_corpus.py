"""The edge-case corpus (tests/golden/edge_lines.json, written by tools/find_edge_lines.py) still says what it claims: every line
is legal from the start position in the oracle, its final position has its category's property (helpers.edge_features), and
every category holds its minimum number of distinct lines."""
import collections

from helpers import EDGE_CATEGORIES, edge_features, load_edge_lines


def test_edge_corpus_lines_are_legal_and_named_right(orc):
    lines = load_edge_lines()
    assert len({e["name"] for e in lines}) == len(lines)
    for e in lines:
        assert e["category"] in EDGE_CATEGORIES and 0 < len(e["uci"]) <= 400, e["name"]
        st = orc.State()
        mv = None
        for u in e["uci"]:
            mv = orc.from_uci(u)
            assert mv in st.legal_moves(), (e["name"], u)
            oc = st.outcome()   # lines run on past claimable draws only, never past a game's automatic end
            assert oc is None or oc["termination"] in ("ThreefoldRepetition", "FiftyMoves"), (e["name"], oc)
            st.push(mv)
        assert e["category"] in edge_features(st, mv), (e["name"], sorted(edge_features(st, mv)))


def test_edge_corpus_category_counts():
    lines = load_edge_lines()
    count = collections.Counter(e["category"] for e in lines)
    distinct = collections.defaultdict(set)
    for e in lines:
        distinct[e["category"]].add(tuple(e["uci"]))
    for cat, n in EDGE_CATEGORIES.items():
        assert len(distinct[cat]) >= n, (cat, count[cat])
