"""Cost of a round against an outside opponent (sc_selfplay_external_wait + sc_selfplay_push_moves) next to the searched ply it sits
between, and next to the same moves applied the only way there was before: one sc_selfplay_set_position per slot with the
lengthened move list.  Prints one JSON line per measured ply and appends them to profiles/external_rate_<date>.jsonl (--out).

  python tools/external_rate.py [--slots 256] [--rollout 60] [--plies 10,100] [--reps 3] [--out FILE]

Synthetic evaluator, the engine Black in every game (so the opponent moves at the even plies), temperature 1 on every ply: long
random-looking games, few of which end before ply 100.  A first pass plays the match against a RandomOpponent and records its
answers; the measured pass replays them from a ScriptedOpponent (the engine is deterministic: the games are the same), so the
opponent's share of a round is one dictionary look-up per move.
Per measured ply P, over the rounds at plies P-4 .. P+4: round_ms = wait_ms + opponent_ms + push_ms (host wall time; both calls
synchronise), search_ply_ms = sc_selfplay_external_search plus the wait for the stream.  set_position_ms: the n moves of the round
at ply P applied to a second, ordinary handle by n sc_selfplay_set_position calls with the n lists of P + 1 moves, --reps times.
All as [median, min, max]."""
import argparse
import time

from ratelib import emit, record, require_device, spread  # sets the package path

import scamd  # noqa: E402
from scamd import external as ext  # noqa: E402


class Recorder:
    """plays as `inner` and keeps every answer: {(game, position line): move}"""
    needs_moves = False

    def __init__(self, inner):
        self.inner, self.table = inner, {}

    def moves(self, requests):
        out = self.inner.moves(requests)
        for r, mv in zip(requests, out):
            self.table[r["game"], ext.position_line(r)] = mv
        return out


def handle(args, external):
    sp = scamd.SelfPlay(None, n_slots=args.slots, n_games=args.slots, rollout_num=args.rollout, num_steps=max(args.plies) + 6, cpuct=1.5,
                        temperature=1.0, temperature_switch=0, with_noise=False, outcome_gate=-1, seed=7, tie_random=True, evaluator="synth")
    if external:
        sp.set_external(None, 0x1111, 2)
    return sp


def med(xs):
    return [round(x, 4) for x in spread(xs)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--rollout", type=int, default=60)
    ap.add_argument("--plies", default="10,100", help="even plies to report, comma separated")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="result file (default profiles/external_rate_<date>.jsonl)")
    args = ap.parse_args()
    args.plies = sorted(int(x) for x in args.plies.split(","))
    if any(p & 1 or p < 0 for p in args.plies):
        raise SystemExit("--plies: the opponent moves at the even plies")
    require_device()
    sp = handle(args, True)
    rec = Recorder(ext.RandomOpponent(seed=3))
    ext.run_external(sp, rec)
    sp.close()
    opp = ext.ScriptedOpponent(rec.table)

    sp, base = handle(args, True), handle(args, False)
    rounds, searches, setpos = {}, {}, {}   # ply -> samples
    ply = -1
    while True:
        while True:
            t0 = time.perf_counter()
            reqs = sp.external_wait()
            t1 = time.perf_counter()
            if not reqs:
                break
            answers = opp.moves(reqs)
            t2 = time.perf_counter()
            ply = reqs[0]["ply"]
            if ply in args.plies:   # (outside the round's clock) the lists a caller without push_moves would replay
                lists = [r["moves"] + [mv] for r, mv in zip(sp.external_wait(moves=True), answers)]
                samples = []
                for _ in range(args.reps):
                    s0 = time.perf_counter()
                    for r, ln in zip(reqs, lists):
                        base.set_position(r["slot"], ln)
                    samples.append((time.perf_counter() - s0) * 1e3)
                setpos[ply] = (len(reqs), samples)
                t2b = time.perf_counter()
            else:
                t2b = t2
            status = sp.push_moves([r["slot"] for r in reqs], answers)
            t3 = time.perf_counter()
            assert min(status) >= 0, status
            rounds.setdefault(ply, []).append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2b) * 1e3, len(reqs)))
        if sp.stats()["games_active"] == 0:
            break
        t0 = time.perf_counter()
        sp.external_search()
        sp.sync()
        searches.setdefault(ply + 1, []).append((time.perf_counter() - t0) * 1e3)   # the ply behind the round's
    stats = sp.stats()
    sp.close()
    base.close()
    lines = []
    for p in args.plies:
        near = [x for q in range(p - 4, p + 5) for x in rounds.get(q, [])]
        if not near or p not in setpos:
            raise SystemExit(f"no game reached ply {p}")
        srch = [x for q in range(p - 4, p + 6) for x in searches.get(q, [])]
        rnd = med([w + o + u for w, o, u, _ in near])
        s = med(srch)
        n, sp_ms = setpos[p]
        lines.append(record("external_rate", slots=args.slots, rollout=args.rollout, ply=p, n_moves=n, rounds=len(near), round_ms=rnd,
                            wait_ms=med([x[0] for x in near]), opponent_ms=med([x[1] for x in near]), push_ms=med([x[2] for x in near]),
                            set_position_ms=med(sp_ms), x_set_position_over_round=round(med(sp_ms)[0] / rnd[0], 2), search_ply_ms=s,
                            round_share_of_ply=round(rnd[0] / s[0], 4), error_flags=stats["error_flags"]))
    emit(lines, args.out, "external_rate")


if __name__ == "__main__":
    main()
