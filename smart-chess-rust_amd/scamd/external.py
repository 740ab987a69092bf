"""Match play against an outside opponent (csrc/external_play.hip, csrc/external_kernels.hip): the reference's `play --black-type
stockfish` (src/play.rs:38-59, 89-142), batched.  The engine's plies are searched on the GPU, many games at once; the opponent's
moves come from an object with `moves(requests) -> [uci, ...]` and are played on the GPU in one call per round.

A request is a dict: slot, game (handle-local index), ply, fen and -- for an opponent whose `needs_moves` is true -- moves, the game
so far as UCI strings.  Opponents here: UciOpponent (a pool of UCI engine processes), ScriptedOpponent (a table), RandomOpponent
(a uniformly random legal move)."""
import os
import select
import subprocess
import threading
import time

import numpy as np

from .binding import EngineError
from .selfplay import SelfPlay, elo


def position_line(request, form="fen"):
    """the UCI `position` command of a request: `position fen <fen>` (the reference's form, src/play.rs:112) or
    `position startpos moves e2e4 ...`"""
    if form == "fen":
        return "position fen " + request["fen"]
    if form == "moves":
        mv = request["moves"]
        return "position startpos" + (" moves " + " ".join(mv) if mv else "")
    raise ValueError("position form must be 'fen' or 'moves'")


class ScriptedOpponent:
    """answers from a table: (game, position line) -> uci move, or position line -> uci move where the game does not matter.  For
    tests and for replaying recorded games (two games can pass through one position and go on differently: key those by game)."""

    def __init__(self, table, position="fen"):
        self.table = dict(table)
        self.position = position
        self.needs_moves = position == "moves"

    def moves(self, requests):
        out = []
        for r in requests:
            line = position_line(r, self.position)
            mv = self.table.get((r["game"], line), self.table.get(line))
            if mv is None:
                raise EngineError(f"game {r['game']}: the script has no answer to '{line}'")
            out.append(mv)
        return out

    def close(self):
        pass


class RandomOpponent:
    """a uniformly random legal move per request (scamd.rules.legal_moves on the requests' FENs): the "does it beat random" baseline"""
    needs_moves = False

    def __init__(self, seed=0, device=0):
        self.rng = np.random.default_rng(seed)
        self.device = device

    def moves(self, requests):
        from .rules import legal_moves
        if not requests:
            return []
        legal = legal_moves([[] for _ in requests], fens=[r["fen"] for r in requests], device=self.device)
        return [row[int(self.rng.integers(len(row)))] for row in legal]

    def close(self):
        pass


class _UciProc:
    """one UCI engine process over pipes; lines are read with a deadline"""

    def __init__(self, cmd):
        self.p = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, close_fds=True)
        self.buf = b""
        self.game = None

    def send(self, line):
        try:
            self.p.stdin.write(line.encode() + b"\n")
            self.p.stdin.flush()
        except (BrokenPipeError, OSError):
            raise EngineError("the UCI engine process has died") from None

    def readline(self, deadline):
        fd = self.p.stdout.fileno()
        while b"\n" not in self.buf:
            left = deadline - time.monotonic()
            if left <= 0 or not select.select([fd], [], [], left)[0]:
                raise TimeoutError
            chunk = os.read(fd, 65536)
            if not chunk:
                raise EngineError("the UCI engine process has died")
            self.buf += chunk
        line, self.buf = self.buf.split(b"\n", 1)
        return line.decode(errors="replace").strip()

    def wait_for(self, word, timeout):
        """read to the first line that starts with `word` and return it"""
        deadline = time.monotonic() + timeout
        while True:
            try:
                line = self.readline(deadline)
            except TimeoutError:
                raise EngineError(f"the UCI engine did not answer '{word}' within {timeout} s") from None
            if line.split(" ", 1)[0] == word:
                return line

    def quit(self):
        try:
            self.send("quit")
        except EngineError:
            pass

    def reap(self, deadline):
        """wait for the process to end, to `deadline` at the most; then it is killed"""
        try:
            self.p.wait(timeout=max(deadline - time.monotonic(), 0.0))
        except subprocess.TimeoutExpired:
            self.p.kill()
            self.p.wait()
        for f in (self.p.stdin, self.p.stdout):
            try:
                f.close()
            except OSError:
                pass


class UciOpponent:
    """A pool of UCI engine processes (Stockfish: the reference's StockfishPlayer, src/play.rs:89-142, `Skill Level` its only
    setting).  cmd: the program and its arguments (a list, or a path).  options: {name: value}, sent as `setoption`.  go: what
    follows `go` (the search limit of every move: `depth 1`, `movetime 100`, `nodes 10000`, ...).  position: 'fen' -- `position fen <fen>`,
    the reference's form -- or 'moves' -- `position startpos moves ...`, which lets the engine see repetitions.
    The requests of a round are dealt over the processes, request i to process i % n_procs, and the replies come back in request
    order.  A timeout, a dead process or `bestmove (none)` raises EngineError, which names the game.
    The processes are started in the constructor.  Construct the pool BEFORE the process makes its first HIP call (before the first
    scamd.Engine or SelfPlay): starting child processes from a process that has initialised the GPU runtime forks its threads' and
    the driver's state, which the runtime does not support.  tools/play_uci.py does so by construction.  n_procs <= 8."""

    def __init__(self, cmd, n_procs=4, options=None, go="depth 1", position="fen", timeout=30.0):
        if not 1 <= n_procs <= 8:
            raise ValueError("UciOpponent: 1 <= n_procs <= 8")
        if position not in ("fen", "moves"):
            raise ValueError("position form must be 'fen' or 'moves'")
        self.cmd = [cmd] if isinstance(cmd, str) else list(cmd)
        self.go, self.position, self.timeout = go, position, float(timeout)
        self.needs_moves = position == "moves"
        self.procs = []
        try:
            for _ in range(n_procs):
                self.procs.append(_UciProc(self.cmd))
            for pr in self.procs:
                pr.send("uci")
                pr.wait_for("uciok", self.timeout)
                for name, value in (options or {}).items():
                    pr.send(f"setoption name {name} value {value}")
                pr.send("isready")
                pr.wait_for("readyok", self.timeout)
        except Exception:
            self.close()
            raise

    def _serve(self, pr, batch, out, errors):
        for i, r in batch:
            try:
                if pr.game != r["game"]:
                    pr.send("ucinewgame")
                    pr.game = r["game"]
                pr.send(position_line(r, self.position))
                pr.send("go " + self.go)
                words = pr.wait_for("bestmove", self.timeout).split()
                if len(words) < 2 or words[1] == "(none)":
                    raise EngineError("the UCI engine answered 'bestmove (none)'")
                out[i] = words[1]
            except EngineError as e:
                errors.append((i, EngineError(f"game {r['game']}: {e} (ply {r['ply']}, {r['fen']})")))
                return

    def moves(self, requests):
        out = [None] * len(requests)
        errors = []
        threads = []
        for k, pr in enumerate(self.procs):
            batch = [(i, r) for i, r in enumerate(requests) if i % len(self.procs) == k]
            if batch:
                t = threading.Thread(target=self._serve, args=(pr, batch, out, errors))
                t.start()
                threads.append(t)
        for t in threads:
            t.join()
        if errors:
            raise min(errors, key=lambda e: e[0])[1]
        return out

    def close(self, grace=1.0):
        """`quit` to every process, then each is waited for (all of them for `grace` seconds together; one that stays is killed)"""
        for pr in self.procs:
            pr.quit()
        deadline = time.monotonic() + grace
        for pr in self.procs:
            pr.reap(deadline)
        self.procs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def play_external(engine, opponent, n_games=100, concurrency=None, rollout=60, cpuct=1.5, temperature=0.0, temperature_switch=0,
                  num_steps=200, seed=0, colours=0, evaluator="net", salt=0, on_round=None):
    """n_games of `engine` against `opponent` on min(concurrency, n_games) recycled slots (SelfPlay.set_external): every game is
    `play`'s loop (src/play.rs:318-343: no noise, outcome after every ply, at most num_steps plies, random tie-break).  colours 0:
    the engine is White in every game, 1: in the even games, 2: in none.
    The round: external_wait -> opponent.moves(requests) -> push_moves, repeated while any slot still waits (a game that starts
    with the opponent as White shows up in a second pass), then one searched ply of every live game.
    -> {"traces": the games in ordinal order, "tally": SelfPlay.match_tally() with a = the engine, "elo": elo of the engine over the
    opponent, "total", "wins", "losses"}.  A move the device refuses raises EngineError with the game, the FEN and the move.
    on_round(sp): called after every searched ply (a driver that drains a trace ring)."""
    slots = n_games if concurrency is None else min(int(concurrency), n_games)
    if slots < 1:
        raise ValueError("play_external: concurrency must be positive")
    sp = SelfPlay(engine, n_slots=slots, n_games=n_games, rollout_num=rollout, num_steps=num_steps, cpuct=cpuct, temperature=temperature,
                  temperature_switch=temperature_switch, with_noise=False, outcome_gate=-1, seed=seed, tie_random=True, evaluator=evaluator)
    try:
        sp.set_external(engine if evaluator == "net" else None, salt, colours)
        run_external(sp, opponent, on_round)
        tally = sp.match_tally()
        traces = [sp.trace(g) for g in range(n_games)]
    finally:
        sp.close()
    wins = tally["a_white"]["White"] + tally["b_white"]["Black"]
    losses = tally["a_white"]["Black"] + tally["b_white"]["White"]
    return {"traces": traces, "tally": tally, "elo": elo(n_games, wins, losses), "total": n_games, "wins": wins, "losses": losses}


def run_external(sp, opponent, on_round=None):
    """the round loop of play_external on a handle after set_external, to the end of its games"""
    needs_moves = bool(getattr(opponent, "needs_moves", False))
    while True:
        while True:
            requests = sp.external_wait(moves=needs_moves)
            if not requests:
                break
            answers = opponent.moves(requests)
            status = sp.push_moves([r["slot"] for r in requests], answers)
            for r, mv, st in zip(requests, answers, status):
                if st < 0:
                    why = "is not legal" if st == -1 else "was refused: the slot does not wait for a move"
                    raise EngineError(f"game {r['game']}: the opponent's move {mv} {why} (ply {r['ply']}, {r['fen']})")
        if on_round is not None:
            on_round(sp)
        if sp.stats()["games_active"] == 0:
            return
        sp.external_search()
