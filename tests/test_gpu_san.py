"""SAN game records on the GPU (-m gpu): sc_encode_san_device, the device parser and the encoder behind it in one call.
The yardstick for every move is helpers.san_to_move over the CPU oracle; the yardstick for every tensor is
sc_encode_steps_device (which the oracle pins, test_gpu_encode_device.py) fed those moves with the reference's ValidationDataset
children: every legal move, count 1 on the move played and 0 elsewhere.  Device buffers come from hipMalloc on the HIP runtime
libsc_engine.so uses (ctypes): this file does not import torch -- the torch interop runs in a child process of its own."""
import json
import os
from collections import Counter

import numpy as np
import pytest

import helpers as H
from san_ref import PINNED_RIVAL, one_hot_steps, san_of, yardstick_moves
from support import GOLD, ROOT, TENSORS, _p, _sizes, assert_bit_equal, dev_per_test, run_san, run_steps, run_torch_child, scamd_gpu  # noqa: F401

pytestmark = pytest.mark.gpu
RESERVED = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def san(scamd):
    import scamd.san as m
    return m


@pytest.fixture(scope="module")
def golden(orc, san):
    """the 60 games of the reference's sample.csv: movetext, winners, the yardstick's moves and the one-hot steps"""
    games, winners = san.read_games_csv(os.path.join(GOLD, "ref_sample_games.csv"))
    moves = [yardstick_moves(orc, g) for g in games]
    return dict(games=games, winners=winners, moves=moves, steps=[one_hot_steps(orc, m) for m in moves])


def test_golden_games_in_one_call(scamd, san, orc, dev, golden):
    games, steps = golden["games"], golden["steps"]
    r = run_san(scamd, san, dev, games)
    assert (r["status"] == 0).all(), r["status"]
    flat = np.asarray([m for g in golden["moves"] for m in g], np.uint16)
    assert r["ply_off"][-1] == flat.size and np.array_equal(r["moves"], flat)
    ref = run_steps(scamd, dev, steps)
    assert (ref["status"] == 0).all()
    assert_bit_equal(r, ref)
    share = np.float32(1.0) / (np.float32(1.0) + np.float32(1e-5))
    assert (r["dist"].sum(1) == share).all() and ((r["dist"] == 0) | (r["dist"] == share)).all()
    assert np.array_equal(r["dist"].argmax(1), [orc.move_index(m, p % 2 == 0) for g in golden["moves"] for p, m in enumerate(g)])


@pytest.mark.parametrize("mirror,layout", [(False, 1), (True, 0), (True, 1)])
def test_layouts_and_mirror(scamd, san, dev, golden, mirror, layout):
    r = run_san(scamd, san, dev, golden["games"][:5], mirror, layout)
    assert (r["status"] == 0).all()
    assert_bit_equal(r, run_steps(scamd, dev, golden["steps"][:5], mirror, layout))


def test_each_output_null_in_turn(scamd, san, dev, golden):
    games = golden["games"][:5]
    full = run_san(scamd, san, dev, games)
    for k in TENSORS + ("moves",):
        r = run_san(scamd, san, dev, games, skip=(k,))
        assert k not in r and (r["status"] == 0).all()
        assert_bit_equal(r, full)
    r = run_san(scamd, san, dev, games, skip=TENSORS)   # plain "SAN -> moves"
    assert set(r) == {"moves", "status", "ply_off"} and (r["status"] == 0).all() and np.array_equal(r["moves"], full["moves"])


# ------------------------------------------------------------------ the edge-line corpus, rendered to SAN
@pytest.mark.parametrize("style", ["min", "over", "noeq"])
def test_edge_lines_rendered_to_san(scamd, san, orc, dev, style):
    lines = [ln["uci"] for ln in H.load_edge_lines()] + [PINNED_RIVAL]
    seen = Counter()
    games, want = [], []
    for uci in lines:
        st = orc.State()
        words, moves = [], []
        for i, u in enumerate(uci):
            m = orc.from_uci(u)
            words.append(("%d. " % (i // 2 + 1) if i % 2 == 0 else "") + san_of(st, m, style, seen))
            st.push(m)
            moves.append(m)
        games.append(" ".join(words))
        want.append(moves)
    for k in ("ep", "castle_k", "castle_q", "promo_capture_check", "underpromo") + (("file_dis", "rank_dis", "pinned_rival") if style != "over" else ()):
        assert seen[k] >= 1, (k, dict(seen))
    assert games[-1].endswith("4. O-O Ne7" if style != "over" else "4. 0-0 Ng8-e7")
    r = run_san(scamd, san, dev, games, skip=TENSORS)
    assert (r["status"] == 0).all(), [(i, int(s), games[i]) for i, s in enumerate(r["status"]) if s]
    assert np.array_equal(r["moves"], np.asarray([m for g in want for m in g], np.uint16))
    if style == "min":   # the yardstick reads this rendering too
        assert [yardstick_moves(orc, g) for g in games[-3:]] == want[-3:]


# ------------------------------------------------------------------ failures
def test_failures_in_one_batch(scamd, san, orc, dev):
    clean = "1. e4 e5 2. Nf3 Nc6 3. Bb5 a6"
    games = [clean,
             "1. e5",                                     # no legal move at ply 0
             "1. e4 e5 2. Nf3 Nf6 3. Nxe5 Nxe5",          # ... at the last ply: no black knight reaches e5
             "1. Nf3 d5 2. d3 d4 3. Nd2 e5",              # both knights reach d2
             "1. e4 Pe5 2. d4",                           # not in the grammar
             "1. e4 Ng8-f6=Q+ 2. d4",                     # 8 characters: the tokenizer's reserved value
             "1. f3 e5 2. g4 Qh4# 3. e4",                 # a token after mate
             ""]                                          # no token at all
    assert int(san.tokenize(games[5])[1]) == RESERVED
    want = [0, -1, -6, 100004, 200001, 200001, -5, 0]
    r = run_san(scamd, san, dev, games)
    assert r["status"].tolist() == want
    solo = run_san(scamd, san, dev, [clean])
    assert_bit_equal(r, solo, rows=slice(0, 6))
    assert_bit_equal(solo, run_steps(scamd, dev, [one_hot_steps(orc, yardstick_moves(orc, clean))]))
    # the plies before a failing one are parsed: game 2's first five moves, game 6's mate
    off = r["ply_off"]
    assert r["moves"][off[2]:off[2] + 5].tolist() == yardstick_moves(orc, "e4 e5 Nf3 Nf6 Nxe5")
    assert r["moves"][off[6]:off[6] + 4].tolist() == yardstick_moves(orc, "f3 e5 g4 Qh4#")
    again = run_san(scamd, san, dev, games)
    assert np.array_equal(again["status"], r["status"])
    assert_bit_equal(again, r)
    # more of the grammar's edge: each word alone, as White's first move
    words = ["e9", "i4", "Ze4", "e4e", "=Q", "e8=K", "Nf3=", "x", "--", "O-O-", "o-o", "Ke1"]
    r = run_san(scamd, san, dev, words, skip=TENSORS)
    assert r["status"].tolist() == [200000] * 11 + [-1]


# ------------------------------------------------------------------ edges
def test_no_games_and_one_ply(scamd, san, orc, dev):
    L = scamd.lib()
    off0 = np.zeros(1, np.uint32)
    bufs = {k: dev.alloc(64) for k in TENSORS + ("moves", "status")}
    rc = L.sc_encode_san_device(None, 0, 0, None, _p(off0), 0, 0, dev.stream, *[bufs[k] for k in TENSORS], bufs["moves"], bufs["status"])
    assert rc == 0
    dev.sync()
    assert all((dev.read(p, (64,), np.uint8) == 0x5a).all() for p in bufs.values())   # nothing is written
    r = run_san(scamd, san, dev, ["1. Nf3"])
    assert r["status"].tolist() == [0] and r["moves"].tolist() == [orc.from_uci("g1f3")] and r["n_legal"].tolist() == [20]
    assert_bit_equal(r, run_steps(scamd, dev, [one_hot_steps(orc, [orc.from_uci("g1f3")])]))


def test_65_games_of_mixed_length(scamd, san, orc, dev, golden):
    """more games than lanes, lengths 0 .. the game's own: prefixes of the golden games as token arrays"""
    toks = [san.tokenize(g) for g in golden["games"]]
    cut = [(7 * i) % (toks[i % 60].size + 1) for i in range(65)]
    games = [toks[i % 60][:cut[i]] for i in range(65)]
    steps = [golden["steps"][i % 60][:cut[i]] for i in range(65)]
    assert 0 in cut and max(cut) > 64
    r = run_san(scamd, san, dev, games)
    assert (r["status"] == 0).all()
    assert_bit_equal(r, run_steps(scamd, dev, steps))


def test_long_knight_shuffle_beside_short_games(scamd, san, orc, dev):
    """300 plies of knight moves: far past the claimable draws (the parser plays on, as read_game does), more than 64 plies, and
    long against the other games of its group"""
    shuffle = " ".join(["Nf3", "Nf6", "Ng1", "Ng8"] * 75)
    games = ["1. e4 e5", shuffle, "1. d4", "1. c4 c5 2. Nc3"]
    moves = [yardstick_moves(orc, g) for g in games]
    assert len(moves[1]) == 300
    r = run_san(scamd, san, dev, games)
    assert (r["status"] == 0).all()
    assert_bit_equal(r, run_steps(scamd, dev, [one_hot_steps(orc, m) for m in moves]))
    off = r["ply_off"]
    rep = r["boards"][off[1]:off[2]].reshape(300, 64, 112)[:, 0, 12:14]   # repetition planes of the position before each ply
    assert rep[:4].sum() == 0 and rep[4:8, 0].all() and rep[8:, 1].all()


def test_two_record_groups_long_game_in_the_first(scamd, san, orc, dev):
    """300 games of which game 150 has 4000 plies: 300 x 4002 position records exceed the walk's budget of 2^20, so the call
    walks two groups of games, the long game among short ones in the first.
    The oracle's State holds 1024 plies, so the yardstick walks the first 1000 plies of the shuffle; every fourth ply the board,
    the side to move, the castling rights (all intact: only knights move) and the ep square (none) are those of four plies before,
    and a SAN word's move and a position's legal moves depend on nothing else, so the yardstick's moves and one-hot steps of the
    1000 plies, which must show that period, are continued with it.  The clocks and repetition planes, which do change, come
    from the device on both sides (run_steps is the tensors' yardstick)."""
    short = ["1. e4 e5", "1. d4", "1. c4 c5 2. Nc3"]
    period = ["Nf3", "Nf6", "Ng1", "Ng8"]
    games = [short[i % 3] for i in range(300)]
    games[150] = " ".join(period * 1000)
    by_text = {g: yardstick_moves(orc, g) for g in short + [" ".join(period * 250)]}
    steps = {g: one_hot_steps(orc, m) for g, m in by_text.items()}
    head, head_steps = by_text.pop(" ".join(period * 250)), steps.pop(" ".join(period * 250))
    assert len(head) == 1000 and head == head[:4] * 250 and head_steps == head_steps[:4] * 250
    by_text[games[150]], steps[games[150]] = head[:4] * 1000, head_steps[:4] * 1000
    moves = [by_text[g] for g in games]
    assert len(moves[150]) == 4000 and 262 * 4002 <= 2 ** 20 < 263 * 4002   # the first group ends behind game 261
    r = run_san(scamd, san, dev, games)
    assert (r["status"] == 0).all(), r["status"]
    assert np.array_equal(r["moves"], np.asarray([m for g in moves for m in g], np.uint16))
    assert_bit_equal(r, run_steps(scamd, dev, [steps[g] for g in games]))


def test_bad_arguments_are_refused(scamd, san, dev):
    L = scamd.lib()
    tokens, off = san.pack_tokens(["1. e4"])
    o = {k: dev.alloc(nb) for k, nb in _sizes(1, 0).items()}
    status = dev.alloc(4)
    host = np.zeros(7168, np.int8)

    def call(**kw):
        a = dict(o, status=status, layout=0, off=_p(off))
        a.update(kw)
        return L.sc_encode_san_device(None, 0, 1, _p(tokens), a["off"], 0, a["layout"], dev.stream, *[a[k] for k in TENSORS], a["moves"],
                                      a["status"])
    assert call(boards=_p(host)) == -1 and "boards" in L.sc_last_error().decode() and "device memory" in L.sc_last_error().decode()
    assert call(moves=_p(host)) == -1 and "moves" in L.sc_last_error().decode()
    assert call(status=_p(host)) == -1 and "status" in L.sc_last_error().decode()
    assert call(status=None) == -1 and call(off=None) == -1 and call(layout=2) == -1
    long_off = np.array([0, 4001], np.uint32)
    assert call(off=_p(long_off)) == -1 and "too long" in L.sc_last_error().decode()   # refused before a token is read
    assert call() == 0   # ... and a good call on the same buffers still works afterwards
    dev.sync()
    assert dev.read(status, (1,), np.int32).tolist() == [0]


# ------------------------------------------------------------------ torch
_CHILD = r'''
import json, sys
import torch                      # first: libsc_engine.so then binds to the runtime torch loaded
sys.path.insert(0, sys.argv[1])
import numpy as np
import scamd
import scamd.san
job = json.load(open(sys.argv[2]))
out = {}
torch.zeros(1, device="cuda:0")
games, winners = scamd.san.read_games_csv(job["csv"], limit=10)
eng = scamd.Engine(2, 128, seed=7)
t = scamd.san.encode_san_torch(games, winners, device=0)
steps = [[(s[0], [tuple(c) for c in s[1]]) for s in g] for g in job["steps"]]
sign = {"white": 1.0, "black": -1.0, "draw": 0.0}
ref = scamd.encode_steps_torch(steps, layout="reference", dist="legal", outcomes=[sign[w] for w in winners])
out["status_ok"] = bool((t["status"] == 0).all() and (ref["status"] == 0).all())
out["moves_equal"] = t["moves"].cpu().numpy().astype(np.uint16).tolist() == [s[0] for g in steps for s in g]
out["tensors_equal"] = bool(all(torch.equal(t[k], ref[k]) for k in ("boards", "meta", "dist_legal", "legal_idx", "n_legal", "outcome"))
                            and t["dist"] is None and np.array_equal(t["ply_off"], ref["ply_off"]))
exp_oc = np.repeat(np.asarray([sign[w] for w in winners], np.float32), np.diff(t["ply_off"].astype(np.int64)))
out["outcome_equal"] = bool(np.array_equal(t["outcome"].cpu().numpy(), exp_oc))
a, b = scamd.score_torch(eng, t), scamd.score_torch(eng, ref)
out["score_equal"] = bool(all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in ("ce", "se", "ent", "value"))
                          and all(a[k] == b[k] for k in ("n", "loss1", "loss2", "pi_entropy", "n_nonfinite")))
out["n"], out["loss1"], out["n_nonfinite"] = a["n"], a["loss1"], a["n_nonfinite"]
c = scamd.compare_torch(eng, eng, t)
out["compare_self"] = [c["n"], c["tv_max"], c["dv_max"]]
eng.close()
torch.cuda.synchronize()
print(json.dumps(out))
'''


def test_torch_scoring_in_a_fresh_process(scamd, golden, tmp_path):
    """torch imported first, then scamd: encode_san_torch on the reference's own ten validation games with their winners, and
    score_torch on that dict, equal score_torch on encode_steps_torch of the yardstick's moves bit for bit"""
    pytest.importorskip("torch")
    job = tmp_path / "job.json"
    job.write_text(json.dumps({"csv": os.path.join(GOLD, "ref_sample_games.csv"), "steps": golden["steps"][:10]}))
    out = run_torch_child(tmp_path, _CHILD, os.path.join(ROOT, "smart-chess-rust_amd"), str(job), timeout=600)
    assert out["status_ok"] and out["moves_equal"] and out["tensors_equal"] and out["outcome_equal"] and out["score_equal"], out
    assert out["n"] == sum(len(g) for g in golden["steps"][:10]) and np.isfinite(out["loss1"]) and out["n_nonfinite"] == 0, out
    assert out["compare_self"] == [out["n"], 0.0, 0.0], out
