"""Evaluation matches between two 10 x 128 bf16 networks at rollout 100 (scripts/leader-board): the lockstep form -- one handle of
n_games slots per colour assignment, sc_selfplay_set_players -- against the recycled form -- one handle of `concurrency` slots
that plays both assignments, sc_selfplay_set_match -- on one box in one session.

  (a) the leader-board match, 100 + 100 games: lockstep, recycled on 200 slots, recycled on 128 slots
  (b) a large match, 1 024 + 1 024 games:      lockstep (two handles of 1 024 slots), recycled on 256 slots
  (o) the leader-board match from opening lines (--openings FILE, a suite of tools/make_openings.py): recycled on 128 slots,
      without the lines and with them (SelfPlay.set_openings: games 2j and 2j + 1 start from line j), and in both rows
      shared_first_20: the games whose first 20 searched plies are those of another game of the match

Each row: simulations/s and wall time of the play phase (first enqueue to the last game's end, traces not fetched), games_active
averaged over the looks at the statistics (one every two plies, as scamd.play_match looks), and the results.  Case (a) also times
the whole scamd.play_match call, traces included.  Rows go to stdout and to --out as JSON lines.

    python tools/match_time.py [--out profiles/match_recycle_<date>.jsonl] [--cases a,b] [--blocks 10] [--rollout 100]
    python tools/match_time.py --cases o --openings openings_2.txt --out profiles/match_openings_<date>.jsonl
"""
import argparse
import datetime
import os
import time

from ratelib import ROOT, emit, require_device  # sets the package path

import scamd  # noqa: E402

SEARCH = dict(cpuct=1.5, temperature=0.0, temperature_switch=0, num_steps=200)


def _handle(engine, n_slots, n_games, rollout, seed):
    return scamd.SelfPlay(engine, n_slots=n_slots, n_games=n_games, rollout_num=rollout, with_noise=False, outcome_gate=-1, seed=seed,
                          tie_random=True, **SEARCH)


def _drive(handles, rollout):
    """scamd.play_match's loop: two plies per look at the statistics -> (seconds, simulations, mean games_active, looks)"""
    live = list(handles)
    active_sum = looks = 0
    t0 = time.perf_counter()
    while live:
        for _ in range(2):
            if len(live) > 1:
                scamd.enqueue_interleaved(live, rollout)
            else:
                live[0].enqueue(rollout)
        stats = [sp.stats() for sp in live]
        active_sum += sum(s["games_active"] for s in stats)
        looks += 1
        live = [sp for sp, s in zip(live, stats) if s["games_active"] > 0]
    dt = time.perf_counter() - t0
    stats = [sp.stats() for sp in handles]
    assert all(s["error_flags"] == 0 for s in stats), stats
    return dt, sum(s["sims_done"] for s in stats), active_sum / max(looks, 1), looks


def _results_from_traces(sp, n_games):
    res = {"White": 0, "Black": 0, "draw": 0, "unfinished": 0}
    for g in range(n_games):
        oc = sp.trace(g)["outcome"]
        res["unfinished" if oc is None else "draw" if oc["winner"] is None else oc["winner"]] += 1
    return res


def lockstep(a, b, n_games, rollout, seed):
    handles = []
    for i, (w, bl) in enumerate(((a, b), (b, a))):
        sp = _handle(w, n_games, n_games, rollout, seed + i)
        sp.set_players(w, bl)
        handles.append(sp)
    dt, sims, active, looks = _drive(handles, rollout)
    res = {"a_white": _results_from_traces(handles[0], n_games), "b_white": _results_from_traces(handles[1], n_games)}
    row = dict(form="lockstep", slots=2 * n_games, launches_per_step=handles[0].launches_per_step())
    for sp in handles:
        sp.close()
    return row, dt, sims, active, looks, res


def shared_prefix(sp, n_games, plies=20):
    """the games whose first `plies` searched plies (the whole game if it is shorter) are those of another game"""
    seen = {}
    for g in range(n_games):
        key = tuple(s[0] for s in sp.trace(g)["steps"][:plies])
        seen[key] = seen.get(key, 0) + 1
    return sum(n for n in seen.values() if n > 1)


def recycled(a, b, n_games, rollout, seed, concurrency, openings=None, count_shared=False):
    sp = _handle(a, min(concurrency, 2 * n_games), 2 * n_games, rollout, seed)
    sp.set_match(a, b, colours=1)
    if openings is not None:
        sp.set_openings(openings)
    dt, sims, active, looks = _drive([sp], rollout)
    res = sp.match_tally()
    row = dict(form="recycled", slots=min(concurrency, 2 * n_games), launches_per_step=sp.launches_per_step())
    if openings is not None:
        row["openings"] = len(openings)
    if count_shared:
        row["shared_first_20"] = shared_prefix(sp, 2 * n_games)
    sp.close()
    return row, dt, sims, active, looks, res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", f"match_recycle_{datetime.date.today():%Y%m%d}.jsonl"))
    ap.add_argument("--cases", default="a,b")
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--rollout", type=int, default=100)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--openings", default=None, help="opening file for case o (tools/make_openings.py)")
    args = ap.parse_args()
    require_device()
    a, b = scamd.Engine(args.blocks, 128, seed=1), scamd.Engine(args.blocks, 128, seed=2)
    plan = {"a": (100, [("lockstep", None), ("recycled", 200), ("recycled", 128)]), "b": (1024, [("lockstep", None), ("recycled", 256)]),
            "o": (100, [("recycled", 128)] + ([("openings", 128)] if args.openings else []))}
    lines = scamd.selfplay.read_openings(args.openings) if args.openings else None
    rows = []
    # (a first, short match warms the device up; it is not reported)
    recycled(a, b, 8, args.rollout, args.seed, 16)
    for case in args.cases.split(","):
        n_games, forms = plan[case]
        for form, conc in forms:
            row, dt, sims, active, looks, res = (lockstep(a, b, n_games, args.rollout, args.seed) if form == "lockstep" else
                                                 recycled(a, b, n_games, args.rollout, args.seed, conc, lines if form == "openings" else None,
                                                          count_shared=case == "o"))
            row = dict(case=case, games=2 * n_games, **row, network=f"{args.blocks}x128 bf16", rollout=args.rollout, play_seconds=round(dt, 3),
                       simulations=sims, sims_per_s=round(sims / dt), games_active_mean=round(active, 1), looks=looks, results=res)
            if case == "a":   # the whole call as a user makes it, traces fetched
                t0 = time.perf_counter()
                scamd.play_match(a, b, n_games=n_games, rollout=args.rollout, seed=args.seed, swap=True, concurrency=conc, **SEARCH)
                row["play_match_seconds"] = round(time.perf_counter() - t0, 3)
            emit([row], args.out, "match_time", mode="a" if rows else "w")   # a run's rows replace the file's
            rows.append(row)
    a.close()
    b.close()


if __name__ == "__main__":
    main()
