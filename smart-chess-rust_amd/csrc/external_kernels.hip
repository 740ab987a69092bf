// external_kernels.hip -- match play against an outside opponent (sc_selfplay_set_external): the kernels of the ply boundary.  The
// opponent's moves are PLAYED in many slots at once (k_push_moves, what StockfishPlayer::bestmove + step do for one game,
// src/play.rs:103-141, 290-316, 335), games are counted and started between two searched plies (k_external_boundary) and the slots
// that wait for the opponent are listed (k_external_wait).  The search kernels know nothing of this: as with recycled match slots
// (mcts_kernels.hip) the host gives them total_games = 0, so a slot whose game ends goes idle.  One wavefront per slot; cold code, a
// handful of launches per ply.  Built with -ffp-contract=off as every unit that includes the search headers.
#include "search_expand.hpp"

#include "launchers.hpp"

namespace sc {
// external_mode: 0 on a handle without an outside opponent, else 1 + colours of sc_selfplay_set_external.  Is the engine White in
// game ordinal k?  colours 0: in every game; 1: in the even ordinals; 2: in none
__device__ inline bool external_engine_white(int external_mode, unsigned long long k) {
    const int colours = external_mode - 1;
    return colours == 0 || (colours == 1 && !(k & 1));
}
// does the slot's game wait for the outside opponent's move at hist[ply]?
__device__ inline bool external_opponent_to_move(const SpParams& p, int external_mode, uint64_t game_id, uint8_t turn) {
    return (turn == WHITE) != external_engine_white(external_mode, game_id - p.first_game_id);
}

// ------------------------------------------------------------------ sc_selfplay_push_moves
// Entry i plays moves[i] in slot slots[i].  status[i]: -2 the slot does not stand at a ply boundary with a fresh root (or, on an
// external handle, the engine is to move), -1 the move is not among the generated legal moves (the 16-bit move as the generator
// emits it), 0 the game goes on, 1 this move ended it.  A refused entry writes nothing but its status.  The ply is recorded as the
// reference records an outside player's ply: every legal move a child, one visit on the move played, values 0.  The advance is the
// end-of-ply code of dev_expand (search_expand.hpp), statement for statement.
__global__ __launch_bounds__(64) void k_push_moves(SpParams p, int n, const int32_t* slots, const uint16_t* moves, int32_t* status,
                                                   int external_mode) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    __shared__ move_t s_moves[MAXC];
    __shared__ Position s_np;
    const int g = uniform(slots[i]);
    if (g < 0 || g >= p.n_slots) {   // (the host has refused these already)
        if (lane == 0) status[i] = -2;
        return;
    }
    GameCtl& c = p.ctl[g];
    const GameCtl cs = uniform(c);
    const size_t nb = (size_t)g * p.node_cap;
    Position* hist = p.hist + (size_t)g * p.hist_cap;
    Position* tpos = p.tpos + (size_t)g * p.tpos_cap;
    const int ply = cs.ply, i_step = cs.ply - cs.start_ply, ts = cs.trace_slot;
    bool ok = cs.status == ST_ACTIVE && cs.sim == 0 && cs.leaf_kind == LK_NONE && cs.n_nodes == 1 && uniform(p.H[nb]).fc == -1;
    ok = ok && ply >= 0 && ply + 1 < p.hist_cap && i_step >= 0 && i_step < p.num_steps && ts >= 0 && ts < p.trace_cap;   // (what the stores below index)
    Position cur{};
    if (ok) {
        cur = uniform(hist[ply]);
        if (external_mode && !external_opponent_to_move(p, external_mode, cs.game_id, cur.turn)) ok = false;
    }
    if (!ok) {
        if (lane == 0) status[i] = -2;
        return;
    }
    const move_t mv = (move_t)uniform((int)moves[i]);
    int nl = 0;
    gen_legal_wave(cur, s_moves, lane, nl);
    __syncthreads();
    if (!legal_has_move(s_moves, nl, mv, lane)) {
        if (lane == 0) status[i] = -1;
        return;
    }
    // the trace step of a ply that was not searched (the root was reset and never visited: q = 0)
    const size_t tstep = (size_t)ts * p.num_steps + (size_t)i_step;
    for (int k = lane; k < nl; k += 64) {
        p.t_cmove[tstep * MAXC + k] = s_moves[k];
        p.t_cn[tstep * MAXC + k] = s_moves[k] == mv ? 1 : 0;
        p.t_cq[tstep * MAXC + k] = 0.0f;
        p.t_cu[tstep * MAXC + k] = 0.0f;
    }
    if (lane == 0) {
        p.t_move[tstep] = mv;
        p.t_q[tstep] = 0.0f;
        p.t_nchild[tstep] = nl;
    }
    // advance the game line
    Position np = cur;
    make_move(np, mv);
    if (lane == 0) s_np = np;
    wave_sync();
    {
        DevChain ch{hist, ply, tpos, nullptr, &s_np, ply + 1};
        uint8_t rf = rep_flags_wave(ch, ply + 1, np.key, lane);
        np.flags = (uint8_t)((np.flags & F_IRREV) | rf);
    }
    wave_sync();
    if (lane == 0) {
        hist[ply + 1] = np;
        atomicAdd(&p.cnt->plies_done, 1ULL);
    }
    wave_sync();
    const int new_ply = ply + 1;
    if (lane == 0) c.ply = new_ply;
    if (i_step > p.outcome_gate) {
        HistChain hc{hist};
        int winner = -1;
        int term = outcome_claim_draw(hc, new_ply, &winner);
        if (term != T_NONE) {
            wave_sync();
            finish_game(p, g, lane, 1, term, winner);
            if (lane == 0) status[i] = 1;
            return;
        }
    }
    if (i_step + 1 >= p.num_steps || new_ply + 1 >= p.hist_cap) {
        wave_sync();
        finish_game(p, g, lane, 0, 0, -1);
        if (lane == 0) status[i] = 1;
        return;
    }
    if (lane == 0) {
        tpos[0] = np;
        p.N[nb] = 0;
        p.W[nb] = 0.0f;
        p.P[nb] = 0.0f;
        p.U[nb] = 0.0f;
        p.MV[nb] = mv;
        p.H[nb] = NodeHdr{-1, 0, 0};
        c.n_nodes = 1;
        c.n_exp = 1;
        c.sim = 0;
        status[i] = 0;
    }
}

// ------------------------------------------------------------------ the boundary of an external handle
// phase 0: k_match_boundary's tally -- int32 [slot][White's player][White won / Black won / draw / no outcome], player 0 the engine,
// 1 the outside opponent; trace_slot < 0 marks the slot as counted.  phase 1 (one wave): every free slot takes the next ordinal, in
// slot order -- ballots, no atomic: which slot plays which game does not depend on the order the waves run in -- and parks it as
// ST_MATCH_WAIT.  phase 2: a parked game starts if its trace-ring row is free (try_start_game), else it stays ST_MATCH_WAIT, which
// the search kernel leaves alone (it retries ST_PENDING in mid-ply).  Any game may start at any boundary: there is no parity rule,
// the side that is to move in the new game moves next.
// The ordinals are counted in cnt->match_next[0]: cnt->next_game is bumped by every finish_game (start_new_game draws from it
// before it finds total_games = 0), so it runs ahead of the games that were started.
__global__ __launch_bounds__(64) void k_external_boundary(SpParams p, int external_mode, int phase) {
    const int g = blockIdx.x, lane = threadIdx.x;
    GameCtl& c = p.ctl[g];
    if (phase == 0) {
        if (lane != 0 || c.status != ST_IDLE || c.trace_slot < 0) return;
        const TraceHdr& th = p.thdr[c.trace_slot];
        const int w = external_engine_white(external_mode, c.game_id - p.first_game_id) ? 0 : 1;
        const int r = !th.has_outcome ? 3 : th.winner == 1 ? 0 : th.winner == 0 ? 1 : 2;
        p.match_tally()[((size_t)g * 2 + w) * 4 + r] += 1;
        c.trace_slot = -1;
        return;
    }
    if (phase == 1) {   // ONE wave: the free slots draw their ordinals in slot order
        const unsigned long long total = (unsigned long long)p.total_games;
        unsigned long long next = p.cnt->match_next[0];
        for (int g0 = 0; g0 < p.n_slots; g0 += 64) {
            const int s = g0 + lane;
            const bool idle = s < p.n_slots && p.ctl[s].status == ST_IDLE;
            const unsigned long long mask = __ballot(idle);
            const unsigned long long k = next + (unsigned long long)__popcll(mask & ((1ULL << lane) - 1ULL));
            if (idle && k < total) {
                p.ctl[s].status = ST_MATCH_WAIT;
                p.ctl[s].leaf_kind = LK_NONE;
                p.ctl[s].game_id = p.first_game_id + k;
            }
            next += (unsigned long long)__popcll(mask);
        }
        if (lane == 0) p.cnt->match_next[0] = next < total ? next : total;
        return;
    }
    if (uniform(c.status) != ST_MATCH_WAIT) return;
    try_start_game(p, g, lane, uniform((bb_t)c.game_id) - p.first_game_id);
    if (lane == 0 && c.status == ST_PENDING) c.status = ST_MATCH_WAIT;
}

// ------------------------------------------------------------------ sc_selfplay_external_wait
// The slots that wait for the opponent -- active, at a ply boundary, the opponent to move -- in ascending slot order: ONE wave walks
// the slots 64 at a time and a ballot gives every waiting slot its place (no atomic counter: the order is the slots').  Entry j:
// list[j] the slot, recs[j] its root record, ep_legal[j] k_fen_ep_legal's bit for it, info[j] = {game ordinal, ply, trace row,
// plies recorded so far}.
__global__ __launch_bounds__(64) void k_external_wait(SpParams p, int external_mode, int32_t* list, int32_t* count, Position* recs,
                                                      int32_t* ep_legal, int4* info) {
    const int lane = threadIdx.x;
    int base = 0;
    for (int g0 = 0; g0 < p.n_slots; g0 += 64) {
        const int g = g0 + lane;
        bool waits = false;
        GameCtl c{};
        if (g < p.n_slots) {
            c = p.ctl[g];
            if (c.status == ST_ACTIVE && c.sim == 0 && c.leaf_kind == LK_NONE && c.ply >= 0 && c.ply < p.hist_cap)
                waits = external_opponent_to_move(p, external_mode, c.game_id, p.hist[(size_t)g * p.hist_cap + c.ply].turn);
        }
        const unsigned long long mask = __ballot(waits);
        if (waits) {
            const int j = base + __popcll(mask & ((1ULL << lane) - 1ULL));
            const Position rec = p.hist[(size_t)g * p.hist_cap + c.ply];
            list[j] = g;
            recs[j] = rec;
            ep_legal[j] = (rec.ep >= 0 && has_legal_ep(rec)) ? 1 : 0;
            info[j] = make_int4((int)(c.game_id - p.first_game_id), c.ply, c.trace_slot, c.ply - c.start_ply);
        }
        base += __popcll(mask);
    }
    if (lane == 0) *count = base;
}

}  // namespace sc

namespace scl {
void push_moves(const sc::SpParams& p, int n, const int32_t* d_slots, const uint16_t* d_moves, int32_t* d_status, int external_mode,
                hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(sc::k_push_moves, dim3(n), dim3(64), 0, s, p, n, d_slots, d_moves, d_status, external_mode);
}
void external_boundary(const sc::SpParams& p, int external_mode, hipStream_t s) {
    hipLaunchKernelGGL(sc::k_external_boundary, dim3(p.n_slots), dim3(64), 0, s, p, external_mode, 0);
    hipLaunchKernelGGL(sc::k_external_boundary, dim3(1), dim3(64), 0, s, p, external_mode, 1);
    hipLaunchKernelGGL(sc::k_external_boundary, dim3(p.n_slots), dim3(64), 0, s, p, external_mode, 2);
}
void external_wait(const sc::SpParams& p, int external_mode, int32_t* d_list, int32_t* d_count, sc::Position* d_recs, int32_t* d_ep_legal,
                   int4* d_info, hipStream_t s) {
    hipLaunchKernelGGL(sc::k_external_wait, dim3(1), dim3(64), 0, s, p, external_mode, d_list, d_count, d_recs, d_ep_legal, d_info);
}
}  // namespace scl
