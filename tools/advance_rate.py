"""Cost and gain of keeping the searched subtree when a move is played (sc_selfplay_advance, SelfPlay.advance).  Prints JSON lines
and appends them to profiles/advance_rate_<date>.jsonl (--out).

  python tools/advance_rate.py [--slots 256] [--rollouts 180,800] [--big 20000,1000000] [--reps 3] [--blocks 10 --channels 128]
                               [--game-moves 10] [--game-nodes 400] [--out FILE]

  kind "call"        one advance call for `slots` slots, each `rollout` simulations into a search of its own (root noise on: the trees
                     differ), into its most-visited child -- next to the same moves through one set_position per slot on a second
                     handle.  The tool checks that both leave the same position in every slot.  [median, min, max] over --reps
  kind "one_slot"    one slot with a tree of at least --big nodes: the one-workgroup sweep at its worst
  kind "kept_share"  what is gained: the share of the root's visits below the most-visited child, and below the most-visited reply
                     after it, as means over the slots -- for the synthetic evaluator and for a random blocks x channels bf16 network
  kind "uci_game"    the UCI engine (scamd.uci.Protocol over LibSearcher, the network) over a scripted game of --game-moves moves,
                     `go nodes --game-nodes` each, without and with KeepTree: simulations per second of search time and the visits kept
Strength is not measured here."""
import argparse
import time

import numpy as np

from ratelib import common_args, emit, record, require_device, spread  # sets the package path

import scamd  # noqa: E402
from scamd import uci  # noqa: E402


def med(xs):
    return [round(x, 4) for x in spread(xs)]


def searched(sp, slots, sims):
    """every slot back at the start position and `sims` simulations into its search -> the report of the trees"""
    for g in range(slots):
        sp.set_position(g, [])
    sp.enqueue(sims)
    sp.sync()
    return sp.report(multipv=1, pv_cap=1)


def call_lines(args):
    out = []
    for R in [int(x) for x in args.rollouts.split(",")]:
        kw = dict(n_slots=args.slots, n_games=args.slots, rollout_num=2 * R + 2, num_steps=150, cpuct=2.5, with_noise=True, seed=7,
                  evaluator="synth", outcome_gate=1 << 30)
        a, b = scamd.SelfPlay(None, **kw), scamd.SelfPlay(None, **kw)
        adv_ms, set_ms, nodes, kept_nodes = [], [], 0, 0
        for k in range(args.reps + 1):
            rep = searched(a, args.slots, R)
            moves = [int(rep["pv"][g, 0, 0]) for g in range(args.slots)]
            t0 = time.perf_counter()
            status, kept = a.advance(list(range(args.slots)), moves)
            adv_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            for g in range(args.slots):
                b.set_position(g, [moves[g]])
            b.sync()
            set_ms.append((time.perf_counter() - t0) * 1e3)
            if status != [0] * args.slots:
                raise SystemExit(f"advance refused or ended {sum(s != 0 for s in status)} slots")
            if any(a.fen(g) != b.fen(g) for g in range(args.slots)):
                raise SystemExit("advance and set_position leave different positions")
            nodes, kept_nodes = int(np.median(rep["n_nodes"])), int(np.median(kept[:, 0]))
        am, sm = med(adv_ms[1:]), med(set_ms[1:])
        out.append(record("advance_rate", kind="call", slots=args.slots, rollout=R, reps=args.reps, nodes_per_slot=nodes, kept_nodes=kept_nodes,
                          advance_ms=am, set_position_ms=sm, x_set_position_over_advance=round(sm[0] / am[0], 3), same_position=True,
                          error_flags=a.stats()["error_flags"] | b.stats()["error_flags"]))
        a.close()
        b.close()
    return out


def one_slot_lines(args):
    out = []
    for target in [int(x) for x in args.big.split(",")]:
        sp = scamd.SelfPlay(None, n_slots=1, n_games=1, rollout_num=60000, num_steps=4000, cpuct=2.5, with_noise=False, seed=7, evaluator="synth",
                            outcome_gate=1 << 30)
        ms, nodes, sims, kept_nodes = [], 0, 0, 0
        for k in range(args.reps + 1):
            sp.set_position(0, [])
            sims, nodes = 0, 1
            while nodes < target and sims + 512 < 59000:
                sp.enqueue(512)
                sims += 512
                nodes = int(sp.report(multipv=1, pv_cap=1)["n_nodes"][0])
            mv = int(sp.report(multipv=1, pv_cap=1)["pv"][0, 0, 0])
            t0 = time.perf_counter()
            status, kept = sp.advance([0], [mv])
            ms.append((time.perf_counter() - t0) * 1e3)
            if status != [0]:
                raise SystemExit(f"advance: status {status}")
            kept_nodes = int(kept[0][0])
        out.append(record("advance_rate", kind="one_slot", target=target, nodes=nodes, sims=sims, kept_nodes=kept_nodes, reps=args.reps,
                          advance_ms=med(ms[1:]), error_flags=sp.stats()["error_flags"]))
        sp.close()
    return out


def kept_share_lines(args, eng):
    out = []
    R = int(args.rollouts.split(",")[0])
    for evaluator, e in (("synth", None), ("net", eng)):
        sp = scamd.SelfPlay(e, n_slots=args.slots, n_games=args.slots, rollout_num=2 * R + 2, num_steps=150, cpuct=2.5, with_noise=True, seed=7,
                            evaluator=evaluator, outcome_gate=1 << 30)
        rep = searched(sp, args.slots, R)
        root = rep["root_n"].astype(np.float64)
        own = rep["line_n"][:, 0].astype(np.float64)
        status, kept = sp.advance(list(range(args.slots)), [int(rep["pv"][g, 0, 0]) for g in range(args.slots)])
        live = np.asarray(status) == 0
        reply = np.zeros(args.slots)   # (the report has no lines before the kept root's first new simulation: the trees themselves)
        for g in np.flatnonzero(live):
            t = sp.tree(int(g))
            fc, nc = int(t["first_child"][0]), int(t["n_child"][0])
            reply[g] = t["n"][fc:fc + nc].max() if fc >= 0 and nc else 0
        out.append(record("advance_rate", kind="kept_share", evaluator=evaluator, slots=args.slots, rollout=R, live=int(live.sum()),
                          network=None if e is None else f"{args.blocks}x{args.channels} bf16, random",
                          share_own_move=round(float((own / root)[live].mean()), 4), share_after_reply=round(float((reply / root)[live].mean()), 4),
                          kept_nodes_mean=round(float(kept[:, 0][live].mean()), 1), error_flags=sp.stats()["error_flags"]))
        sp.close()
    return out


def uci_game_lines(args, eng):
    out = []
    for keep in (False, True):
        lines_out = []
        proto = uci.Protocol(uci.LibSearcher(eng), lines_out.append)
        proto.opt["KeepTree"] = keep
        proto.opt["Chunk"] = 4096
        moves, search_s, kept_visits = [], 0.0, 0
        for _ in range(args.game_moves):
            del lines_out[:]
            proto.handle("position startpos" + (" moves " + " ".join(moves) if moves else ""))
            t0 = time.perf_counter()
            proto.handle(f"go nodes {args.game_nodes}")
            search_s += time.perf_counter() - t0
            kept_visits += sum(int(ln.split()[5]) for ln in lines_out if ln.startswith("info string kept"))
            best = [ln.split()[1] for ln in lines_out if ln.startswith("bestmove")][0]
            if best == "0000":
                break
            moves.append(best)
        flags = proto.s.sp.stats()["error_flags"]
        proto.s.close()
        sims = len(moves) * args.game_nodes
        out.append(record("advance_rate", kind="uci_game", keep_tree=keep, moves=len(moves), nodes_per_move=args.game_nodes,
                          network=f"{args.blocks}x{args.channels} bf16, random", nps=round(sims / search_s, 1), kept_visits=kept_visits,
                          visits_per_move=round((sims + kept_visits) / max(len(moves), 1), 1), error_flags=flags))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--rollouts", default="180,800")
    ap.add_argument("--big", default="20000,1000000", help="node counts of the one-slot trees, comma separated")
    ap.add_argument("--game-moves", type=int, default=10)
    ap.add_argument("--game-nodes", type=int, default=400)
    ap.add_argument("--out", default=None, help="result file (default profiles/advance_rate_<date>.jsonl)")
    common_args(ap, reps=3)
    args = ap.parse_args()
    require_device()
    lines = call_lines(args) + one_slot_lines(args)
    eng = scamd.Engine(args.blocks, args.channels, seed=1)
    lines += kept_share_lines(args, eng) + uci_game_lines(args, eng)
    eng.close()
    emit(lines, args.out, "advance_rate")


if __name__ == "__main__":
    main()
