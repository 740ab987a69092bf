"""Batched self-play, searches, interactive play and matches (csrc/selfplay.hip, csrc/match_play.hip, csrc/selfplay_io.hip); the two debug hooks (csrc/debug_calls.hip)."""
import ctypes as C
import math

import numpy as np

from .binding import (EVALUATORS, MAX_MOVES, TERMINATION, EngineError, SelfplayConfig, Stats, TraceInfo, _check, _count, _Handle,
                      _moves, _p, _stream, _torch, lib, move_uci)
from .net import ChessHip, encode_positions
from .training import _device_outputs, _finish_outputs


class SelfPlay(_Handle):
    """Batched `selfplay` (src/main.rs): same option names as the reference CLI (main.rs:25-60)."""
    _destroy = "sc_selfplay_destroy"

    def __init__(self, engine=None, n_slots=256, n_games=None, rollout_num=180, num_steps=150, cpuct=2.5,
                 temperature=0.0, temperature_switch=4, epsilon=0.15, with_noise=True, outcome_gate=100,
                 evaluator="net", external_noise=False, seed=0, first_game_id=0, trace_capacity=0, own_stream=False, device=0,
                 tie_random=False, trace_hold=False, rollout_factor=0.0):
        self.L = lib()
        self.engine = engine
        self.device = engine.device if engine is not None else device
        self.cfg = cfg = SelfplayConfig(n_slots, n_games if n_games is not None else n_slots, rollout_num, num_steps, cpuct,
                                        temperature, temperature_switch, epsilon, int(with_noise), outcome_gate,
                                        EVALUATORS[evaluator], int(external_noise), seed, first_game_id, trace_capacity, int(own_stream),
                                        int(tie_random), int(trace_hold), float(rollout_factor))
        self.h = h = C.c_void_p()
        _check(self.L.sc_selfplay_create(engine.h if engine else None, device, C.byref(cfg), C.byref(h)))

    def enqueue(self, n_sims):
        _check(self.L.sc_selfplay_enqueue_sims(self.h, n_sims))

    def set_players(self, white=None, black=None, salt_white=0, salt_black=0):
        """match play (src/play.rs:318-343): even plies are searched by `white`, odd plies by `black`"""
        self._players = (white, black)   # keep the engines alive
        _check(self.L.sc_selfplay_set_players(self.h, white.h if white else None, black.h if black else None, salt_white, salt_black))

    def set_match(self, a=None, b=None, salt_a=0, salt_b=0, colours=1):
        """match play with slot recycling (sc_selfplay_set_match): n_games games on n_slots slots; colours=1: `a` is White in
        the even games of the handle and `b` in the odd ones, colours=0: `a` in all of them"""
        self._players = (a, b)   # keep the engines alive
        _check(self.L.sc_selfplay_set_match(self.h, a.h if a else None, b.h if b else None, salt_a, salt_b, colours))

    def set_external(self, engine=None, salt=0, colours=0):
        """an outside opponent (sc_selfplay_set_external): the handle searches the engine's plies only -- colours 0: the engine is
        White in every game, 1: in the even games, 2: in none -- and is stepped by external_wait / push_moves / external_search
        (scamd.external.play_external is the loop)"""
        self._players = (engine,)   # keep the engine alive
        _check(self.L.sc_selfplay_set_external(self.h, engine.h if engine else None, salt, colours))

    def external_search(self):
        """sc_selfplay_external_search: one searched ply of every live game, enqueued; refused while a slot waits for the opponent"""
        _check(self.L.sc_selfplay_external_search(self.h))

    def external_wait(self, moves=False):
        """sc_selfplay_external_wait: the slots that wait for the opponent's move, in slot order -> list of dicts with slot, game
        (handle-local), ply, fen and, with moves=True, the game's moves so far as UCI strings"""
        G = self.cfg.n_slots
        slots, games, plies = (np.zeros(G, np.int32) for _ in range(3))
        fens, foff = np.zeros(G * 96, np.uint8), np.zeros(G + 1, np.uint32)
        mcap = G * self.cfg.num_steps if moves else 0
        mv, moff = np.zeros(max(mcap, 1), np.uint16), np.zeros(G + 1, np.uint32)
        n = _count(self.L.sc_selfplay_external_wait(self.h, G, _p(slots), _p(games), _p(plies), _p(fens), fens.size, _p(foff),
                                                    _p(mv) if moves else None, mcap, _p(moff) if moves else None))
        text = fens.tobytes()
        out = []
        for i in range(n):
            r = dict(slot=int(slots[i]), game=int(games[i]), ply=int(plies[i]), fen=text[foff[i]:foff[i + 1] - 1].decode())
            if moves:
                r["moves"] = [move_uci(m) for m in mv[moff[i]:moff[i + 1]]]
            out.append(r)
        return out

    def push_moves(self, slots, moves):
        """sc_selfplay_push_moves: plays moves[i] (UCI string or uint16) in slot slots[i] -> status per entry: 0 the game goes on,
        1 the move ended it, -1 not a legal move, -2 the slot does not stand at a ply boundary with the pusher to move"""
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        n = slots.size
        if len(moves) != n:
            raise ValueError("one move per slot")
        status = np.zeros(max(n, 1), np.int32)
        _count(self.L.sc_selfplay_push_moves(self.h, n, _p(slots) if n else None, _p(_moves(moves)) if n else None, _p(status)))
        return [int(x) for x in status[:n]]

    def advance(self, slots, moves):
        """sc_selfplay_advance: plays moves[i] (UCI string or uint16) in slot slots[i] and keeps the searched subtree below it: the
        chosen root child becomes the root and the next enqueue goes on from it -> (status, kept): status per entry 0 the game goes
        on, 1 the move ended it, -1 the move is not among the root's children (root not searched: the legal moves), -2 the slot
        is not active or has a simulation in flight; kept int32 [n][3]: n_nodes, n_exp and the new root's visits"""
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        n = slots.size
        if len(moves) != n:
            raise ValueError("one move per slot")
        status = np.zeros(max(n, 1), np.int32)
        kept = np.zeros((max(n, 1), 3), np.int32)
        _count(self.L.sc_selfplay_advance(self.h, n, _p(slots) if n else None, _p(_moves(moves)) if n else None, _p(status), _p(kept)))
        return [int(x) for x in status[:n]], kept[:n]

    def set_openings(self, lines):
        """sc_selfplay_set_openings: game k of a match handle starts from line opening_of_game(k, len(lines), colours); a line
        is a list of UCI strings or uint16 moves (empty: the start position), or a pair (fen, moves): the moves start from that
        position (sc_selfplay_set_openings_from).  Raises EngineError with .status, the per-line codes (0 ok, -(j+1): move j is
        not legal, 1: the line's last position ends the game; for a base that cannot be used, its scamd.fen.Positions status),
        when the call is refused."""
        from .fen import bases_of
        fens = [ln[0] if _is_fen_line(ln) else None for ln in lines]
        lines = [ln[1] if _is_fen_line(ln) else ln for ln in lines]
        lines = [_moves(ln)[:len(ln)] for ln in lines]
        off = np.zeros(len(lines) + 1, np.uint32)
        off[1:] = np.cumsum([ln.size for ln in lines])
        mv = np.ascontiguousarray(np.concatenate(lines + [np.zeros(1, np.uint16)]), np.uint16)
        status = np.zeros(max(len(lines), 1), np.int32)
        pos, bidx, owned = bases_of(fens, len(lines), self.device)
        try:
            if pos is None:
                rc = self.L.sc_selfplay_set_openings(self.h, len(lines), _p(mv), _p(off), _p(status))
            else:
                rc = self.L.sc_selfplay_set_openings_from(self.h, len(lines), pos.h, _p(bidx), _p(mv), _p(off), _p(status))
            err = self.L.sc_last_error().decode() if rc != 0 else ""
        finally:
            if owned:
                pos.close()   # (the handle keeps its own records of the lines)
        if rc != 0:
            e = EngineError(f"libsc_engine error {rc}: {err}")
            e.code, e.status = rc, [int(x) for x in status[:len(lines)]]
            raise e

    def get_opening(self, game):
        """sc_selfplay_get_opening: the line handle-local game `game` starts from, as UCI strings"""
        n = _count(self.L.sc_selfplay_get_opening(self.h, game, None, 0))
        buf = np.zeros(max(n, 1), np.uint16)
        _count(self.L.sc_selfplay_get_opening(self.h, game, _p(buf), n))
        return [move_uci(m) for m in buf[:n]]

    def get_opening_fen(self, game):
        """sc_selfplay_get_opening_fen: the position the line of handle-local game `game` starts from, None for the start position"""
        buf = C.create_string_buffer(128)
        n = _count(self.L.sc_selfplay_get_opening_fen(self.h, game, buf, 128))
        return buf.value.decode() if n else None

    def fen(self, slot):
        """sc_selfplay_get_fen: python-chess's Board.fen() of the slot's current position"""
        buf = C.create_string_buffer(128)
        _count(self.L.sc_selfplay_get_fen(self.h, slot, buf, 128))
        return buf.value.decode()

    def match_tally(self):
        """sc_selfplay_match_tally: the games finished so far, by the player that was White and by result"""
        out = np.zeros(8, np.int64)
        _check(self.L.sc_selfplay_match_tally(self.h, _p(out)))
        return {key: dict(zip(("White", "Black", "draw", "unfinished"), (int(x) for x in out[4 * w:4 * w + 4])))
                for w, key in enumerate(("a_white", "b_white"))}

    def sync(self):
        _check(self.L.sc_selfplay_synchronize(self.h))

    def run(self, max_sim_steps=0):
        _check(self.L.sc_selfplay_run(self.h, max_sim_steps))

    def stats(self):
        s = Stats()
        _check(self.L.sc_selfplay_get_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in Stats._fields_}

    def enable_timing(self, stride=1):
        _check(self.L.sc_selfplay_enable_timing(self.h, stride))

    def check_flags(self, what):
        """raises EngineError (.code -4, .flags) if the handle's error flags are set (sc_selfplay_stats.error_flags: 8 = a descent
        reached the depth limit of 1024 path nodes): the trees of a flagged handle are not those of the search, as sc_search
        refuses them"""
        flags = self.stats()["error_flags"]
        if flags:
            e = EngineError(f"{what}: search error flags {flags} set (1 non-finite PUCT value, 2 node pool overflow, 4 move without "
                            "action index, 8 path deeper than 1024 nodes, 16 / 32 hand-off timeout): the tree is invalid")
            e.code, e.flags = -4, flags
            raise e

    def launches_per_step(self):
        """1: fused step kernel with the value FC inside, 2: fused step kernel + value FC launch, 3: separate launches"""
        return int(self.L.sc_selfplay_launches_per_step(self.h))

    def timing(self, reset=True):
        a, b, n = C.c_float(0), C.c_float(0), C.c_int64(0)
        _check(self.L.sc_selfplay_timing(self.h, int(reset), C.byref(a), C.byref(b), C.byref(n)))
        return dict(ms_total=a.value, ms_tower_sum=b.value, tower_launches=n.value)

    def poll(self, cap=4096):
        """sc_selfplay_poll: handle-local indices of the games that finished since they were last reported"""
        buf = np.zeros(max(cap, 1), np.int32)
        n = _count(self.L.sc_selfplay_poll(self.h, _p(buf), cap))
        return [int(x) for x in buf[:n]]

    def trace(self, game):
        """-> dict in the reference's trace-file shape (src/trace.rs:5-9); None if unfinished; raises EngineError when the
        trace has left the device (ring row overwritten or released)"""
        info = TraceInfo()
        rc = self.L.sc_selfplay_get_trace(self.h, game, C.byref(info), None, None, None, None, None, None, None)
        if rc == 1:
            return None
        _check(rc)
        ns, nc = info.n_steps, info.n_children_total
        sm, sq = np.zeros(ns + 1, np.uint16), np.zeros(ns + 1, np.float32)
        co = np.zeros(ns + 2, np.int32)
        cm, cn = np.zeros(nc + 1, np.uint16), np.zeros(nc + 1, np.int32)
        cq, cu = np.zeros(nc + 1, np.float32), np.zeros(nc + 1, np.float32)
        _check(self.L.sc_selfplay_get_trace(self.h, game, C.byref(info), _p(sm), _p(sq), _p(co), _p(cm), _p(cn), _p(cq),
                                            _p(cu)))
        steps = []
        for i in range(ns):
            ch = [(move_uci(cm[j]), int(cn[j]), float(cq[j]), float(cu[j])) for j in range(co[i], co[i + 1])]
            steps.append((move_uci(sm[i]), float(sq[i]), ch))
        outcome = None
        if info.has_outcome:
            outcome = {"termination": TERMINATION[info.termination], "winner": {1: "White", 0: "Black", -1: None}[info.winner]}
        return {"steps": steps, "outcome": outcome, "game_id": int(info.game_id)}

    def training_tensors(self, games, apply_mirror=False, layout="trainer", dist="dense"):
        """Training tensors of finished games straight from the trace ring (sc_selfplay_encode_traces), as torch tensors on
        this handle's GPU -- see encode_steps_torch for the result.  outcome comes from the ring headers.  Raises EngineError
        with .code 1 if a game has not finished, 2 if its ring row has been overwritten or released."""
        games = np.ascontiguousarray(games, np.int32).reshape(-1)
        n = games.size
        torch = _torch()
        ply_off = np.zeros(n + 1, np.uint32)
        _check(self.L.sc_selfplay_encode_traces(self.h, n, _p(games), 0, 0, None, _p(ply_off), None, None, None, None, None,
                                                None, None))
        win = np.zeros(n, np.float32)
        info = TraceInfo()
        for i, g in enumerate(games):
            _check(self.L.sc_selfplay_get_trace(self.h, int(g), C.byref(info), None, None, None, None, None, None, None))
            win[i] = {1: 1.0, 0: -1.0}.get(info.winner, 0.0) if info.has_outcome else 0.0
        out, args = _device_outputs(torch, self.device, int(ply_off[n]), n, layout, dist)
        _check(self.L.sc_selfplay_encode_traces(self.h, n, _p(games), int(bool(apply_mirror)), args[0], _stream(torch, self.device),
                                                _p(ply_off), *args[1:]))
        return _finish_outputs(torch, out, ply_off, win, apply_mirror, self.device)

    def write_trace(self, game, path):
        _check(self.L.sc_selfplay_write_trace_json(self.h, game, path.encode()))

    def traces_json(self, games):
        """sc_selfplay_traces_json: the trace-file text of finished games (handle-local indices), formatted on the GPU from the
        trace ring in one call -> list of bytes, each what write_trace writes for the game.  Raises EngineError with .code 1 if
        a game has not finished, 2 if its ring row has been overwritten or released."""
        games = list(games)
        g = np.ascontiguousarray(games or [0], np.int32)
        n = len(games)
        off = np.zeros(n + 1, np.uint64)
        _check(self.L.sc_selfplay_traces_json(self.h, n, _p(g), None, 0, _p(off)))
        text = np.zeros(max(int(off[n]), 1), np.uint8)
        _check(self.L.sc_selfplay_traces_json(self.h, n, _p(g), _p(text), int(off[n]), _p(off)))
        return [text[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)]

    def write_traces(self, games, paths):
        """sc_selfplay_write_traces_json: the files write_trace writes for `games`, formatted on the GPU in one call"""
        games, paths = list(games), [p.encode() for p in paths]
        if len(games) != len(paths):
            raise ValueError("one path per game")
        g = np.ascontiguousarray(games or [0], np.int32)
        arr = (C.c_char_p * max(len(paths), 1))(*paths)
        _check(self.L.sc_selfplay_write_traces_json(self.h, len(games), _p(g), arr))

    def write_pgn(self, games, path, append=False, white=None, black=None, event=None):
        """finished games (handle-local indices) as PGN, rendered on the GPU in one call (sc_selfplay_write_pgn)"""
        games = list(games)
        g = np.asarray(games or [0], np.int32)
        names = [None if x is None else x.encode() for x in (white, black, event)]
        _check(self.L.sc_selfplay_write_pgn(self.h, len(games), _p(g), path.encode(), int(bool(append)), *names))

    def stream_traces(self, path_of, chunk=None):
        """The loop of lib/sc-selfplay (src/main.rs:235-238 writes each game's file when it ends): plays every game of the
        handle and writes `path_of(game_id)` as games finish, from a handle created with a trace ring and trace_hold=True.
        The next ply's simulation steps are enqueued BEFORE the finished games' traces are fetched and written: a reported
        row is final, it is read while the GPU searches.  -> number of files written."""
        chunk = chunk or self.cfg.rollout_num
        written = 0
        self.enqueue(chunk)
        while True:
            fin = self.poll()
            active = self.stats()["games_active"]
            if active:
                self.enqueue(chunk)
            if fin:   # the round's games in one call, formatted on the GPU from their held rows
                self.write_traces(fin, [path_of(self.cfg.first_game_id + g) for g in fin])
                written += len(fin)
            if not active and not fin:
                return written

    def tree(self, slot, cap=1 << 20):
        n = min(_count(self.L.sc_selfplay_get_tree(self.h, slot, 0, None, None, None, None, None, None, None)), cap)
        out = dict(n=np.zeros(n, np.int32), q=np.zeros(n, np.float32), uct=np.zeros(n, np.float32),
                   prior=np.zeros(n, np.float32), move=np.zeros(n, np.uint16), first_child=np.zeros(n, np.int32),
                   n_child=np.zeros(n, np.int32))
        _count(self.L.sc_selfplay_get_tree(self.h, slot, n, _p(out["n"]), _p(out["q"]), _p(out["uct"]), _p(out["prior"]),
                                           _p(out["move"]), _p(out["first_child"]), _p(out["n_child"])))
        return out

    def report(self, slots=None, multipv=1, pv_cap=64):
        """sc_selfplay_report: what the searches of `slots` (None: all) found, read on the GPU in one launch and one copy -> a
        scamd.report.Report: a dict of numpy arrays (status, ply, sim, n_nodes, n_root_children, root_children_n, root_n, root_w,
        turn, n_lines per entry; line_child, line_n, line_w, line_prior, line_len, line_end [n][multipv]; pv [n][multipv][pv_cap])
        whose lines(i) gives entry i's lines by visits as dicts with move, pv, n, q, prior, len, end and score"""
        from .report import report
        return report(self, slots, multipv, pv_cap)

    def debug_cycles(self, enable=True, read=False):
        """sc_selfplay_debug_cycles: switch the stamps on / read those of the last launch -> uint64[n_slots, 32] (or None)"""
        out = np.zeros((self.cfg.n_slots, 32), np.uint64) if read else None
        _check(self.L.sc_selfplay_debug_cycles(self.h, int(enable), _p(out)))
        return out

    def slot(self, slot):
        ply, sim, st, plen = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        gid = C.c_uint64(0)
        path = np.zeros(1024, np.int32)
        _check(self.L.sc_selfplay_get_slot(self.h, slot, C.byref(ply), C.byref(sim), C.byref(st), C.byref(gid), _p(path),
                                           C.byref(plen)))
        return dict(ply=ply.value, sim=sim.value, status=st.value, game_id=gid.value, path=path[:plen.value].copy())

    def set_noise(self, slot, noise):
        noise = np.ascontiguousarray(noise, np.float32)
        _check(self.L.sc_selfplay_set_noise(self.h, slot, _p(noise), noise.size))

    def get_noise(self, slot, n):
        out = np.zeros(MAX_MOVES, np.float32)
        _check(self.L.sc_selfplay_get_noise(self.h, slot, _p(out), MAX_MOVES))
        return out[:n]

    def set_position(self, slot, moves, fen=None):
        """sc_selfplay_set_position(_from): the slot starts from `moves` played from the start position, or from `fen`: a FEN
        string, or (scamd.fen.Positions, index) to share one validated set among many calls"""
        if fen is None:
            _check(self.L.sc_selfplay_set_position(self.h, slot, _p(_moves(moves)), len(moves)))
            return
        from .fen import Positions
        pos, i = fen if isinstance(fen, tuple) else (Positions([fen], self.device), 0)
        try:
            _check(self.L.sc_selfplay_set_position_from(self.h, slot, pos.h, i, _p(_moves(moves)), len(moves)))
        finally:
            if not isinstance(fen, tuple):
                pos.close()


def enqueue_interleaved(handles, n_sims):
    """n simulation steps on several SelfPlay handles (own_stream=True), interleaved step by step"""
    arr = (C.c_void_p * len(handles))(*[h.h for h in handles])
    _check(lib().sc_selfplay_enqueue_interleaved(arr, len(handles), n_sims))


def search(engine, moves, rollout, cpuct=2.5, noise=False, seed=0, fen=None):
    """sc_search(_from): one search from the position after `moves`, played from the start position or from `fen`
    -> (root_q, [(uci, N, Q, prior), ...])"""
    mv = _moves(moves)
    cm, cn = np.zeros(MAX_MOVES, np.uint16), np.zeros(MAX_MOVES, np.int32)
    cq, cp = np.zeros(MAX_MOVES, np.float32), np.zeros(MAX_MOVES, np.float32)
    rq = C.c_float(0)
    if fen is None:
        n = _count(lib().sc_search(engine.h, _p(mv), len(moves), rollout, cpuct, int(bool(noise)), seed, MAX_MOVES, _p(cm), _p(cn), _p(cq),
                                   _p(cp), C.byref(rq)))
    else:
        from .fen import Positions
        pos = Positions([fen], engine.device)
        try:
            n = _count(lib().sc_search_from(engine.h, pos.h, 0, _p(mv), len(moves), rollout, cpuct, int(bool(noise)), seed, MAX_MOVES,
                                            _p(cm), _p(cn), _p(cq), _p(cp), C.byref(rq)))
        finally:
            pos.close()
    return rq.value, [(move_uci(cm[i]), int(cn[i]), float(cq[i]), float(cp[i])) for i in range(n)]


class Play:
    """Interactive engine handle: the `chess_play_*` functions of the reference's Python extension
    (src/lib.rs:161-358: new / mcts / step / apply_move / inspect / dump_search_tree / inference / encode) on one
    search slot of the GPU engine.  Differences: moves are UCI strings; `inspect()` returns the move list instead of a
    python-chess board object; the tree keeps only the current subtree (the reference also keeps the never revisited
    siblings of played moves), so `dump_search_tree()` shows the played line as a chain of single children."""

    def __init__(self, engine, initial_moves=(), fen=None, evaluator="net", seed=0, keep_tree=False):
        """fen: the position `initial_moves` start from (a FEN string; None: the start position).  keep_tree: apply_move keeps the
        searched subtree below the move (SelfPlay.advance) instead of starting from a fresh node; a move the tree refuses -- or one
        that ends the game -- falls back to the fresh node.  The pool holds 60 000 evaluations per game then, not per search."""
        self.keep_tree = bool(keep_tree)
        self.engine = engine
        self.moves = [m if isinstance(m, str) else move_uci(m) for m in initial_moves]
        self._seed = seed
        self._base = None
        self._black_base = 0
        if fen is not None:
            from .fen import Positions
            self._base = Positions([fen], engine.device if engine is not None else 0).check(for_search=True)
            self.base_fen = self._base.fen(0)
            self._black_base = int(self.base_fen.split()[1] == "b")
        # rollout_num is the per-ply budget of the self-play driver: huge here, plies advance only through step()
        self.sp = SelfPlay(engine, n_slots=1, n_games=1, rollout_num=60000, num_steps=4000, with_noise=False, outcome_gate=1 << 30,
                           evaluator=evaluator, seed=seed)
        self._rng = np.random.default_rng(seed)
        self._set_position()

    def _set_position(self):
        self.sp.set_position(0, self.moves, fen=None if self._base is None else (self._base, 0))

    def close(self):
        self.sp.close()
        if self._base is not None:
            self._base.close()

    def fen(self):
        """python-chess's Board.fen() of the current position (sc_selfplay_get_fen)"""
        return self.sp.fen(0)

    def mcts(self, rollout, cpuct=2.5, noise=False):
        """chess_play_mcts: `rollout` more simulations on the current tree (epsilon 0.15 as lib.rs:243).  Raises EngineError when
        the search sets an error flag (a path of more than 1024 nodes: a blocked position searched that deep)"""
        _check(self.sp.L.sc_selfplay_set_search(self.sp.h, cpuct, 0.15, int(bool(noise))))
        self.sp.enqueue(rollout)
        self.sp.sync()
        self.sp.check_flags("Play.mcts")

    def _root_children(self):
        t = self.sp.tree(0)
        if t["n"].size == 0 or t["n_child"][0] == 0:
            return t, 0, 0
        return t, int(t["first_child"][0]), int(t["n_child"][0])

    def step(self, temp=0.0):
        """chess_play_step = mcts::step (src/mcts.rs:292-328): temperature 0 -> first most-visited child, else a
        sample ~ N^(1/temp); descends and starts a fresh tree there.  Returns the move or None (no children)."""
        t, fc, nc = self._root_children()
        if nc == 0:
            return None
        n = t["n"][fc:fc + nc].astype(np.float32)
        if temp == 0.0:
            choice = int(np.argmax(n))
        else:
            w = n ** np.float32(1.0 / temp)
            choice = int(self._rng.choice(nc, p=(w / w.sum()).astype(np.float64)))
        mv = move_uci(t["move"][fc + choice])
        self.apply_move(mv)
        return mv

    def apply_move(self, mov):
        """chess_play_apply_move: play `mov` and continue from a fresh node -- with keep_tree from the searched subtree below it"""
        mov = mov if isinstance(mov, str) else move_uci(mov)
        kept = self.keep_tree and self.sp.advance([0], [mov])[0][0] == 0
        self.moves.append(mov)
        if not kept:
            self._set_position()

    def inspect(self):
        """chess_play_inspect -> (None, move stack newest first, q_value of the current node, [(move, N, Q), ...])"""
        t, fc, nc = self._root_children()
        q = float(t["q"][0]) if t["q"].size else 0.0
        ch = [(move_uci(t["move"][fc + i]), int(t["n"][fc + i]), float(t["q"][fc + i])) for i in range(nc)]
        return None, list(reversed(self.moves)), q, ch

    def dump_search_tree(self):
        """chess_play_dump_search_tree: nested dicts with serde's field names (src/mcts.rs:43-56: step, depth, q,
        num_act, children); step = [uci or None, colour of the side to move at the node]; depth counts from the base, whose
        side to move is the root's colour"""
        t = self.sp.tree(0)
        d0 = len(self.moves)
        bb = self._black_base

        def node(i, depth, mv):
            colour = "White" if (depth + bb) % 2 == 0 else "Black"
            fc, nc = int(t["first_child"][i]), int(t["n_child"][i])
            kids = [node(fc + k, depth + 1, move_uci(t["move"][fc + k])) for k in range(nc)] if fc >= 0 else []
            return {"step": [mv, colour], "depth": depth, "q": float(t["q"][i]), "num_act": int(t["n"][i]), "children": kids}
        cur = node(0, d0, self.moves[-1] if self.moves else None) if t["n"].size else None
        for d in range(d0 - 1, -1, -1):   # the played line above the current node
            cur = {"step": [self.moves[d - 1] if d > 0 else None, "White" if (d + bb) % 2 == 0 else "Black"], "depth": d, "q": 0.0,
                   "num_act": 0, "children": [cur]}
        return cur

    def inference(self):
        """chess_play_inference -> (legal moves, priors, value) of the current position (Game::predict)"""
        steps, pri, val = ChessHip(self.engine).predict(self.moves, fen=None if self._base is None else self.base_fen)
        return [move_uci(m) for m in steps], pri, val

    def encode(self):
        """chess_play_encode -> (boards int8[8,8,112], meta int32[7])"""
        e = encode_positions([self.moves], engine=self.engine, fens=None if self._base is None else [self.base_fen])
        return e["boards"][0], e["meta"][0]


def elo(total, wins, losses):
    """scripts/elo.py:15-21: Elo difference from Total/Win/Lost"""
    s = (wins + (total - wins - losses) / 2) / total
    if s <= 0.0 or s >= 1.0:
        return math.copysign(math.inf, s - 0.5)
    return 400 * math.log(s / (1 - s), 10)


def opening_of_game(k, n_lines, colours):
    """the line handle-local game k starts from (sc_selfplay_set_openings): with alternating colours games 2j and 2j + 1 share
    line j % n_lines, so every line is played once with each player as White; otherwise game k plays line k % n_lines"""
    return ((k >> 1) if colours else k) % n_lines


def _is_fen_line(ln):
    """an opening line given as (fen, moves)"""
    return isinstance(ln, tuple) and len(ln) == 2 and isinstance(ln[0], str) and "/" in ln[0] and not isinstance(ln[1], str)


def read_openings(path):
    """An opening file -> list of lines (lists of UCI strings).  One line per opening: UCI moves separated by blanks; `#` starts
    a comment (a line that holds nothing but a comment is skipped); an empty line is the start position.  A line whose first word
    is `fen` is `fen <the 4 or 6 fields> [moves m1 m2 ...]`, the UCI `position` convention, and yields (fen, [uci, ...])."""
    import re
    lines = []
    with open(path) as f:
        for no, raw in enumerate(f, 1):
            text = raw.split("#", 1)[0]
            if "#" in raw and not text.strip():
                continue
            toks = text.split()
            fen = None
            if toks and toks[0] == "fen":
                cut = toks.index("moves") if "moves" in toks else len(toks)
                fen, toks = " ".join(toks[1:cut]), toks[cut + 1:]
                if len(fen.split()) not in (4, 6):
                    raise ValueError(f"{path}:{no}: a FEN of 4 or 6 fields is expected behind 'fen'")
                from .fen import parse_fen
                try:
                    parse_fen(fen)
                except ValueError as e:
                    raise ValueError(f"{path}:{no}: {e}") from None
            for t in toks:
                if not re.fullmatch(r"[a-h][1-8][a-h][1-8][nbrq]?", t):
                    raise ValueError(f"{path}:{no}: '{t}' is not a UCI move")
            lines.append(toks if fen is None else (fen, toks))
    return lines


def play_match(a, b, n_games=100, rollout=100, cpuct=1.5, temperature=0.0, temperature_switch=0, num_steps=200, seed=0,
               swap=True, concurrency=None, openings=None):
    """Batched `scripts/leader-board:44-54`: n_games with engine `a` as White and `b` as Black, then (swap) the same
    number with the colours exchanged; every game is `play`'s loop (src/play.rs:241-343: no noise, outcome after every
    ply, at most 200 plies, random tie-break).  -> dict(results per colour assignment, a's score, Elo of a over b).
    concurrency=C: all games in ONE handle of min(C, games) recycled slots (SelfPlay.set_match): a finished game's slot goes
    on with the next game, `a` is White in the handle's even games (as_white) and, with swap, `b` in the odd ones (as_black);
    results come from the device's tally.  None: one lockstep handle of n_games slots per colour assignment.
    openings: lines (SelfPlay.set_openings) the games start from -- with swap each line is played once with each engine as White;
    needs the recycled form (concurrency None: one slot per game)."""
    if openings is not None and concurrency is None:
        concurrency = 2 * n_games if swap else n_games
    if concurrency is not None:
        return _play_match_recycled(a, b, n_games, rollout, cpuct, temperature, temperature_switch, num_steps, seed, swap, int(concurrency),
                                    openings)
    out = {"as_white": None, "as_black": None}
    tot = win = lost = 0
    # Both colour assignments play at the same time: each handle launches on the stream of its White engine, so the two sets of
    # n_games workgroups share the GPU (100 + 100 of 256 CUs for the reference's 100-game matches) instead of running one after the
    # other.  A game depends only on its seed and id: the results are those of the sequential loop.
    handles = []
    for key, (w, bl) in (("as_white", (a, b)), ("as_black", (b, a))):
        if key == "as_black" and not swap:
            break
        sp = SelfPlay(w, n_slots=n_games, n_games=n_games, rollout_num=rollout, num_steps=num_steps, cpuct=cpuct,
                      temperature=temperature, temperature_switch=temperature_switch, with_noise=False, outcome_gate=-1,
                      seed=seed + (0 if key == "as_white" else 1), tie_random=True)
        sp.set_players(w, bl)
        handles.append((key, sp))
    live = [sp for _, sp in handles]
    while live:
        for _ in range(2):                       # two plies per look at the statistics
            if len(live) > 1:
                enqueue_interleaved(live, rollout)
            else:
                live[0].enqueue(rollout)
        live = [sp for sp in live if sp.stats()["games_active"] > 0]
    for key, sp in handles:
        res = {"White": 0, "Black": 0, "draw": 0, "unfinished": 0}
        traces = []
        for g in range(n_games):
            t = sp.trace(g)
            traces.append(t)
            oc = t["outcome"] if t else None
            if oc is None:
                res["unfinished"] += 1
            elif oc["winner"] is None:
                res["draw"] += 1
            else:
                res[oc["winner"]] += 1
        sp.close()
        out[key] = dict(results=res, traces=traces)
        a_col, b_col = ("White", "Black") if key == "as_white" else ("Black", "White")
        tot += n_games
        win += res[a_col]
        lost += res[b_col]
    out.update(total=tot, a_wins=win, b_wins=lost, elo_a_minus_b=elo(tot, win, lost))
    return out


def _play_match_recycled(a, b, n_games, rollout, cpuct, temperature, temperature_switch, num_steps, seed, swap, concurrency, openings=None):
    total = 2 * n_games if swap else n_games
    if concurrency < 1:
        raise ValueError("play_match: concurrency must be positive")
    sp = SelfPlay(a, n_slots=min(concurrency, total), n_games=total, rollout_num=rollout, num_steps=num_steps, cpuct=cpuct,
                  temperature=temperature, temperature_switch=temperature_switch, with_noise=False, outcome_gate=-1, seed=seed,
                  tie_random=True)
    sp.set_match(a, b, colours=1 if swap else 0)
    if openings is not None:
        sp.set_openings(openings)
    while True:
        sp.enqueue(2 * rollout)                  # two plies per look at the statistics
        if sp.stats()["games_active"] == 0:
            break
    tally = sp.match_tally()
    stride = 2 if swap else 1
    out = {"as_white": dict(results=tally["a_white"], traces=[sp.trace(g) for g in range(0, total, stride)]), "as_black": None}
    win, lost = tally["a_white"]["White"], tally["a_white"]["Black"]
    if swap:
        out["as_black"] = dict(results=tally["b_white"], traces=[sp.trace(g) for g in range(1, total, 2)])
        win += tally["b_white"]["Black"]
        lost += tally["b_white"]["White"]
    sp.close()
    out.update(total=total, a_wins=win, b_wins=lost, elo_a_minus_b=elo(total, win, lost))
    return out


def write_trace_json(path, trace):
    """sc_trace_write_json on a trace dict (no GPU needed)."""
    steps = trace["steps"]
    ns = len(steps)
    info = TraceInfo()
    info.n_steps = ns
    oc = trace.get("outcome")
    info.has_outcome = int(oc is not None)
    info.termination = {v: k for k, v in TERMINATION.items()}[oc["termination"]] if oc else 0
    info.winner = {"White": 1, "Black": 0, None: -1}[oc["winner"]] if oc else -1
    sm = _moves([s[0] for s in steps] + [0])
    sq = np.asarray([s[1] for s in steps] + [0], np.float32)
    co = np.zeros(ns + 2, np.int32)
    co[1:ns + 1] = np.cumsum([len(s[2]) for s in steps])
    ch = [c for s in steps for c in s[2]]
    info.n_children_total = len(ch)
    cm = _moves([c[0] for c in ch] + [0])
    cn = np.asarray([c[1] for c in ch] + [0], np.int32)
    cq = np.asarray([c[2] for c in ch] + [0], np.float32)
    cu = np.asarray([c[3] for c in ch] + [0], np.float32)
    _check(lib().sc_trace_write_json(path.encode(), C.byref(info), _p(sm), _p(sq), _p(co), _p(cm), _p(cn), _p(cq), _p(cu)))


def find_max(values, device=0):
    """sc_debug_find_max: (one-round result or -2, four-round result) of the descent's arg-max on `values`"""
    v = np.ascontiguousarray(values, np.float32)
    out = np.zeros(2, np.int32)
    _check(lib().sc_debug_find_max(device, _p(v), v.size, _p(out)))
    return int(out[0]), int(out[1])


def choose_child(n_act, nc, temperature, u, tie_random=False, device=0):
    """sc_debug_choose_child: (choice [n] int32, total [n] float32) of the end-of-ply move choice on n cases;
    n_act [n][224] visit counts, nc / temperature / u one value per case"""
    nc = np.ascontiguousarray(nc, np.int32)
    n = nc.size
    n_act = np.ascontiguousarray(n_act, np.int32)
    temperature = np.ascontiguousarray(temperature, np.float32)
    u = np.ascontiguousarray(u, np.float32)
    if n_act.shape != (n, MAX_MOVES) or temperature.shape != (n,) or u.shape != (n,):
        raise ValueError("choose_child: n_act must be [n][224], nc / temperature / u [n]")
    choice = np.zeros(n, np.int32)
    total = np.zeros(n, np.float32)
    _check(lib().sc_debug_choose_child(device, n, _p(n_act), _p(nc), _p(temperature), _p(u), int(tie_random), _p(choice), _p(total)))
    return choice, total
