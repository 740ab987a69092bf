"""The reference's `play --black-type stockfish` (src/play.rs:38-59, 437-446; scripts/tournament), batched: a network against a UCI
engine, many games at once on recycled slots (scamd.external.play_external's loop).

  python tools/play_uci.py --white-device cuda -w net.scw --black-type stockfish --stockfish-bin /usr/bin/stockfish \
      --stockfish-level 0 -r 60 --temperature 0 --temperature-switch 0 --cpuct 1.5 -o 'trace_{}.json' \
      [--games 100] [--concurrency 64] [--swap] [--pgn match.pgn]

The reference's flags keep their names and defaults; `{}` in -o is the game's number, 1 .. games.  The batched extras are those of
sc-play: --games, --concurrency (slots; default: one per game), --swap (the network is White in the odd-numbered games and Black in
the even-numbered ones; without it White in all), --pgn.  Further: --procs (UCI processes, at most 8), --go (the search limit sent
with every `go`), --position fen|moves, --stockfish-arg (an argument for the engine program; repeatable), --blocks / --channels /
--white-seed (a random network when no checkpoint is given), --evaluator synth with --salt (the synthetic evaluator: tests).
The UCI processes are started FIRST, before the GPU is opened: a process that has initialised the HIP runtime should not fork.
Prints one summary line: the tally by the network's colour and the input of scripts/elo.py (Total/Win/Lost of the network)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smart-chess-rust_amd"))

from scamd import external as ext  # noqa: E402  (loads no library and opens no device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--white-device", required=True)
    ap.add_argument("-w", "--white-checkpoint", default=None)
    ap.add_argument("--black-type", default="stockfish", choices=["stockfish"], help="a network as opponent: lib/sc-play")
    ap.add_argument("--stockfish-bin", default="/usr/bin/stockfish")
    ap.add_argument("--stockfish-level", type=int, default=0)
    ap.add_argument("--stockfish-arg", action="append", default=[])
    ap.add_argument("-r", "--rollout", type=int, default=60)
    ap.add_argument("--temperature", type=float, default=0.0)
    ap.add_argument("--temperature-switch", type=int, default=0)
    ap.add_argument("--cpuct", type=float, default=0.0)
    ap.add_argument("-o", "--output", default="01.json")
    ap.add_argument("--games", type=int, default=1)
    ap.add_argument("--concurrency", type=int, default=None)
    ap.add_argument("--swap", action="store_true")
    ap.add_argument("--pgn", default=None)
    ap.add_argument("--procs", type=int, default=4)
    ap.add_argument("--go", default="depth 1")
    ap.add_argument("--position", default="fen", choices=["fen", "moves"])
    ap.add_argument("--timeout", type=float, default=30.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--white-seed", type=int, default=1)
    ap.add_argument("--evaluator", default="net", choices=["net", "synth"])
    ap.add_argument("--salt", type=lambda s: int(s, 0), default=0)
    a = ap.parse_args()
    if not a.white_device.startswith("cuda"):
        raise SystemExit("--white-device: the engine runs on the GPU only (cuda)")
    if a.games < 1 or (a.games > 1 and "{}" not in a.output):
        raise SystemExit("-o needs a {} for the game's number when --games is above 1")

    # 1) the pool, before anything touches the GPU
    opponent = ext.UciOpponent([a.stockfish_bin] + a.stockfish_arg, n_procs=min(a.procs, a.games), options={"Skill Level": a.stockfish_level},
                               go=a.go, position=a.position, timeout=a.timeout)
    try:
        # 2) the engine and the handle
        import scamd
        if scamd.lib().sc_device_count() <= 0:
            raise SystemExit("no HIP device")
        eng = None
        if a.evaluator == "net":
            eng = scamd.Engine(a.blocks, a.channels, seed=a.white_seed, weights=a.white_checkpoint)
        slots = a.games if a.concurrency is None else max(1, min(a.concurrency, a.games))
        sp = scamd.SelfPlay(eng, n_slots=slots, n_games=a.games, rollout_num=a.rollout, num_steps=200, cpuct=a.cpuct, temperature=a.temperature,
                            temperature_switch=a.temperature_switch, with_noise=False, outcome_gate=-1, seed=a.seed, tie_random=True,
                            evaluator=a.evaluator)
        sp.set_external(eng, a.salt, 1 if a.swap else 0)
        ext.run_external(sp, opponent)
    finally:
        opponent.close()
    games = list(range(a.games))
    sp.write_traces(games, [a.output.replace("{}", str(k + 1)) for k in games])
    name = os.path.basename(a.white_checkpoint) if a.white_checkpoint else f"net-seed{a.white_seed}" if eng else f"synth-{a.salt:#x}"
    if a.pgn:
        sp.write_pgn(games, a.pgn, white=name, black=os.path.basename(a.stockfish_bin) + f"-level{a.stockfish_level}", event="play_uci match")
    tally, stats = sp.match_tally(), sp.stats()
    sp.close()
    if eng:
        eng.close()
    w, b = tally["a_white"], tally["b_white"]
    wins, losses = w["White"] + b["Black"], w["Black"] + b["White"]
    line = f"games {a.games} slots {slots} as-white: white-wins {w['White']} black-wins {w['Black']} draws {w['draw']} unfinished {w['unfinished']}"
    if a.swap:
        line += f"  as-black: white-wins {b['White']} black-wins {b['Black']} draws {b['draw']} unfinished {b['unfinished']}"
    print(line + f"   (elo.py input: {a.games}/{wins}/{losses})")
    return 1 if stats["error_flags"] else 0


if __name__ == "__main__":
    sys.exit(main())
