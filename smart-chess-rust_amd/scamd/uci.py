"""The engine behind UCI: a line-oriented front end over one interactive search handle (tools/uci_engine.py wires it to the
library), so that a GUI, a tournament manager or scamd.external.UciOpponent can drive the engine.

Protocol takes its searcher as an argument -- an object with new_game(), set_position(fen, moves), start(cpuct), run(n) -> error
flags, report(multipv) -> dict(sim, lines) and close() -- and is tested without a GPU.  LibSearcher is the searcher over the
library: one slot, a node pool for 60 000 simulations, built like scamd.Play.

Every `go` starts from a fresh one-node tree, as the reference discards the subtree between moves (src/mcts.rs:319-323): `go nodes
N` gives the result of sc_search for the same position, cpuct and evaluator, noise off.  With the option KeepTree the tree lives
on instead: a `position` with the current base whose move list extends the current one is applied by advancing move by move
(searcher.advance(move) -> (nodes, visits) kept, or None: the tree refuses the move and the position is set up afresh), answered
with `info string kept <nodes> nodes <visits> visits`, and `go nodes N` runs N MORE simulations on what was kept.  Any other
`position`, and `ucinewgame`, restart.  The search runs in chunks of `Chunk`
simulations; between chunks the engine drains the reader's queue (`stop`, `quit`, `isready`), looks at the clock and, at most once
per `InfoEvery` milliseconds and always before `bestmove`, prints one `info` line per MultiPV rank from the device's report."""
import queue
import re
import time

MAX_NODES = 59999          # the node pool holds a search of 60 000 simulations
START_FEN = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
OPTIONS = {"MultiPV": ("spin", 1, 1, 224), "CPuct": ("string", "2.5"), "Chunk": ("spin", 64, 1, 4096), "InfoEvery": ("spin", 500, 0, 3600000),
           "KeepTree": ("check", "false")}
_MOVE = re.compile(r"[a-h][1-8][a-h][1-8][nbrq]?$")


def allocate_ms(remaining, inc, movestogo):
    """milliseconds for this move from the clock: remaining / max(movestogo, 30) + inc / 2, at most half of what remains"""
    return min(remaining / max(movestogo, 30) + inc / 2, remaining / 2)


def parse_position(words):
    """the words behind `position` -> (fen or None for startpos, [uci moves]); ValueError names what is wrong"""
    if not words:
        raise ValueError("position: startpos or fen expected")
    cut = words.index("moves") if "moves" in words else len(words)
    head, moves = words[:cut], words[cut + 1:]
    if head[0] == "startpos" and len(head) == 1:
        fen = None
    elif head[0] == "fen" and len(head) in (5, 7):
        fen = " ".join(head[1:])
    else:
        raise ValueError("position: startpos or fen <4 or 6 fields> expected")
    for m in moves:
        if not _MOVE.match(m):
            raise ValueError(f"position: '{m}' is not a UCI move")
    return fen, moves


def parse_go(words):
    """the words behind `go` -> dict of the integer limits given (nodes, movetime, wtime, btime, winc, binc, movestogo, depth) and
    infinite=True; words the engine does not know are skipped"""
    out, i = {}, 0
    while i < len(words):
        w = words[i]
        if w == "infinite":
            out["infinite"] = True
        elif w in ("nodes", "movetime", "wtime", "btime", "winc", "binc", "movestogo", "depth") and i + 1 < len(words):
            try:
                out[w] = int(words[i + 1])
            except ValueError:
                raise ValueError(f"go: {w} needs a number") from None
            i += 1
        i += 1
    return out


def info_line(rank, line, depth, sim, ms):
    """one `info` line of rank `rank` (1 ..) from a report's line"""
    kind, v = line["score"]
    nps = int(sim * 1000 / ms) if ms > 0 else 0
    return f"info depth {depth} multipv {rank} nodes {sim} nps {nps} time {int(ms)} score {kind} {v} pv {' '.join(line['pv'])}"


class Protocol:
    """UCI over a searcher.  write(text): one line out; clock(): seconds.  run(q) serves the lines of queue q (None: end of input)
    until `quit`; handle(line, q) serves one."""

    def __init__(self, searcher, write, clock=time.monotonic, name="smart-chess MI355X", author="the smart-chess-rust_amd authors"):
        self.s, self.write, self.clock, self.name, self.author = searcher, write, clock, name, author
        self.opt = {"MultiPV": 1, "CPuct": 2.5, "Chunk": 64, "InfoEvery": 500}
        if hasattr(searcher, "advance"):   # KeepTree is offered by a searcher that can keep its tree
            self.opt["KeepTree"] = False
        self.fen, self.moves = None, []
        self.live = False   # KeepTree: the searcher holds a searched tree of (self.fen, self.moves)
        self.black_to_move = False
        self.quit = False
        self.pending = []   # commands that arrived during a search, served after it
        self.s.set_position(None, [])

    def run(self, q):
        while not self.quit:
            line = self.pending.pop(0) if self.pending else q.get()
            if line is None:
                break
            self.handle(line, q)
        self.s.close()
        return 0

    def handle(self, line, q=None):
        words = line.split()
        if not words:
            return
        cmd, rest = words[0], words[1:]
        try:
            if cmd == "uci":
                self.write(f"id name {self.name}")
                self.write(f"id author {self.author}")
                for k, spec in OPTIONS.items():
                    if k not in self.opt:
                        continue
                    self.write(f"option name {k} type spin default {spec[1]} min {spec[2]} max {spec[3]}" if spec[0] == "spin"
                               else f"option name {k} type check default {str(bool(self.opt[k])).lower()}" if spec[0] == "check"
                               else f"option name {k} type string default {spec[1]}")
                self.write("uciok")
            elif cmd == "isready":
                self.write("readyok")
            elif cmd == "ucinewgame":
                self.s.new_game()
                self.live = False
            elif cmd == "setoption":
                self._setoption(rest)
            elif cmd == "position":
                fen, moves = parse_position(rest)
                extends = self.live and fen == self.fen and len(moves) > len(self.moves) and moves[:len(self.moves)] == self.moves
                done = self.moves
                self.fen, self.moves = fen, moves
                base_black = self.fen is not None and self.fen.split()[1] == "b"
                self.black_to_move = base_black != bool(len(self.moves) & 1)
                self.live = extends and self._advance(moves[len(done):])
                if not self.live:
                    self.s.set_position(self.fen, self.moves)
            elif cmd == "go":
                self._go(parse_go(rest), q if q is not None else queue.Queue())
            elif cmd == "quit":
                self.quit = True
            # `stop` outside a search, and anything unknown, is ignored, as the protocol asks
        except ValueError as e:
            self.write(f"info string {e}")

    def _advance(self, moves):
        """KeepTree: the searcher's tree follows `moves`, move by move -> False as soon as it refuses one"""
        kept = None
        for m in moves:
            kept = self.s.advance(m)
            if kept is None:
                return False
        self.write(f"info string kept {kept[0]} nodes {kept[1]} visits")
        return True

    def _setoption(self, words):
        if "name" not in words or "value" not in words:
            raise ValueError("setoption name <id> value <x> expected")
        name = " ".join(words[words.index("name") + 1:words.index("value")])
        value = " ".join(words[words.index("value") + 1:])
        key = {k.lower(): k for k in self.opt}.get(name.lower())
        if key is None:
            raise ValueError(f"setoption: no option '{name}'")
        spec = OPTIONS[key]
        if spec[0] == "spin":
            v = int(value)
            if not spec[2] <= v <= spec[3]:
                raise ValueError(f"setoption: {key} must lie in {spec[2]} .. {spec[3]}")
        elif spec[0] == "check":
            if value.lower() not in ("true", "false"):
                raise ValueError(f"setoption: {key} must be true or false")
            v = value.lower() == "true"
            self.live = False
        else:
            v = float(value)
            if not v > 0:
                raise ValueError(f"setoption: {key} must be positive")
        self.opt[key] = v

    def _limits(self, go):
        """-> (simulations at most, milliseconds at most or None, wait for `stop` before answering)"""
        nodes = min(go.get("nodes", MAX_NODES), MAX_NODES)
        ms = go.get("movetime")
        side = "b" if self.black_to_move else "w"
        if ms is None and side + "time" in go:
            ms = allocate_ms(max(go[side + "time"], 0), go.get(side + "inc", 0), go.get("movestogo", 0))
        infinite = bool(go.get("infinite")) or ("nodes" not in go and ms is None)
        return max(nodes, 1), ms, infinite

    def _drain(self, q, block=False):
        """the commands that arrived during a search: True when the search has to end.  `stop`, `quit` and `isready` act at once;
        any other command waits in self.pending for the search's end, and so does everything behind it (a later `stop` is
        not this search's); a search without a limit ends there"""
        while not self.pending:
            try:
                line = q.get(block)
            except queue.Empty:
                return False
            if line is None:
                self.pending.append("quit")   # the end of input: a search with a limit still runs to it
                break
            words = line.split()
            if words[:1] == ["stop"]:
                return True
            if words[:1] == ["quit"]:
                self.quit = True
                return True
            if words[:1] == ["isready"]:
                self.write("readyok")
            elif words:
                self.pending.append(line)
        return block

    def _go(self, go, q):
        nodes, ms, infinite = self._limits(go)
        t0 = self.clock()
        elapsed = lambda: (self.clock() - t0) * 1000.0   # noqa: E731
        if self.opt.get("KeepTree"):
            self.s.start(self.opt["CPuct"], self.live)   # (a live tree is searched on)
            self.live = True
        else:
            self.s.start(self.opt["CPuct"])
        last, last_info, stopped = None, None, False
        done = 0
        while done < nodes and not stopped:
            k = min(self.opt["Chunk"], nodes - done)
            flags = self.s.run(k)
            if flags:
                self.write(f"info string search error flags {flags} (8: a path deeper than 1024 nodes): the answer is the last clean report's")
                break
            done += k
            last = self.s.report(self.opt["MultiPV"])
            if not last["lines"]:
                break   # no legal move
            stopped = self._drain(q)
            now = elapsed()
            if ms is not None and now >= ms:
                stopped = True
            if not stopped and done < nodes and (last_info is None or now - last_info >= self.opt["InfoEvery"]):
                self._info(last, now)
                last_info = now
        if infinite and not stopped and not self.quit:
            self._drain(q, block=True)   # `go infinite` answers only when told to
        if last is not None and last["lines"]:
            self._info(last, elapsed())
            self.write(f"bestmove {last['lines'][0]['move']}")
        else:
            self.write("bestmove 0000")

    def _info(self, rep, ms):
        depth = rep["lines"][0]["len"]
        for k, line in enumerate(rep["lines"], 1):
            self.write(info_line(k, line, depth, rep["sim"], ms))


class LibSearcher:
    """the searcher over the library: one interactive slot (a SelfPlay handle built like scamd.Play's).  evaluator: "net" with
    `engine`, or a synthetic one with `salt` (tests)"""

    def __init__(self, engine=None, evaluator="net", salt=0, seed=0, device=0):
        self.engine, self.evaluator, self.salt, self.seed = engine, evaluator, salt, seed
        self.device = engine.device if engine is not None else device
        self.sp, self.base, self.moves, self.dirty, self.over = None, None, [], False, False
        self.used = 1   # an upper bound of the handle's position records in use (n_exp): kept ones and the simulations since
        self._open()

    def _open(self):
        from .selfplay import SelfPlay
        if self.sp is not None:
            self.sp.close()
        self.sp = SelfPlay(self.engine, n_slots=1, n_games=1, rollout_num=60000, num_steps=4000, with_noise=False, outcome_gate=1 << 30,
                           evaluator=self.evaluator, seed=self.seed, device=self.device)
        if self.evaluator != "net" and self.salt:
            self.sp.set_players(None, None, self.salt, self.salt)
        self.dirty = False

    def new_game(self):
        pass   # (every search starts from a fresh tree anyway)

    def set_position(self, fen, moves):
        from .fen import Positions
        base = None
        if fen is not None:
            base = Positions([fen], self.device)
            if base.status[0] < 0:
                st = int(base.status[0])
                base.close()
                from .fen import STATUS_TEXT
                raise ValueError(f"position: {STATUS_TEXT.get(st, st)}")
        if self.base is not None:
            self.base.close()
        self.base, self.moves = base, list(moves)

    def advance(self, move):
        """plays `move` on the live tree (SelfPlay.advance) -> (nodes, visits) kept, or None: the tree refuses the move, the move
        ends the game or the handle is flagged, and the caller sets the position up afresh"""
        if self.over or self.dirty:
            return None
        st, kept = self.sp.advance([0], [move])
        if st[0] != 0:
            return None
        self.moves.append(move)
        self.used = int(kept[0][1])
        return int(kept[0][0]), int(kept[0][2])

    def start(self, cpuct, live=False):
        """live: the handle's tree is the current position's (a search ran there, or advance led there) and is searched on"""
        from .binding import _check
        # a base where the game is over (mate, stalemate) cannot be searched: there is no move to report
        self.over = self.base is not None and int(self.base.status[0]) == 1 and not self.moves
        if self.over:
            return
        if self.dirty:
            self._open()   # the error flags of a handle stay: a flagged search leaves a new one behind
            live = False
        # the whole move list goes to the handle (chess_play_new's way): the search sees the game's repetitions
        if not live:
            self.sp.set_position(0, self.moves, fen=None if self.base is None else (self.base, 0))
            self.used = 1
        _check(self.sp.L.sc_selfplay_set_search(self.sp.h, cpuct, 0.15, 0))

    def run(self, n):
        if self.over:
            return 0
        # the pool holds MAX_NODES + 1 position records: per search, and per game where trees are kept
        n = min(n, MAX_NODES + 1 - self.used)
        if n <= 0:
            return 0
        self.used += n
        self.sp.enqueue(n)
        self.sp.sync()
        flags = self.sp.stats()["error_flags"]
        self.dirty = self.dirty or bool(flags)
        return flags

    def report(self, multipv):
        if self.over:
            return dict(sim=0, lines=[])
        rep = self.sp.report(multipv=multipv, pv_cap=64)
        return dict(sim=int(rep["sim"][0]), lines=rep.lines(0))

    def close(self):
        if self.sp is not None:
            self.sp.close()
            self.sp = None
        if self.base is not None:
            self.base.close()
            self.base = None
