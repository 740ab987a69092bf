// mcts_kernels.hip -- the unfused search kernel k_mcts, slot setup and the test aids, with their launchers.  Built with
// -ffp-contract=off (search_select.hpp).
#include "search_expand.hpp"

#include "launchers.hpp"

namespace sc {
// ------------------------------------------------------------------ find_max on given values (test aid, sc_debug_find_max)
// The two argmax forms of the descent on caller-provided PUCT values: out[0] = one-round form (n <= 64, lane = child),
// out[1] = four-round (value, index) pair form (n <= 256, lane owns children lane, lane+64, ...), exactly as `level`
// of dev_select combines them.  Lets a test place exact ties, -0.0 / +0.0 pairs and maxima in any lane and round.
__global__ __launch_bounds__(64) void k_debug_find_max(const float* u, int n, int* out) {
    const int lane = threadIdx.x;
    if (n <= 64) {
        const int r = wave_argmax_last_lane(lane < n ? u[lane] : 0.f, lane < n);
        if (lane == 0) out[0] = r;
    } else if (lane == 0) {
        out[0] = -2;
    }
    float best_u = 0.f;
    int best_i = -1;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int i = lane + 64 * r;
        if (i < n) {
            const float v = u[i];
            if (best_i < 0 || v >= best_u) {
                best_u = v;
                best_i = i;
            }
        }
    }
    const int r4 = wave_argmax_last(best_u, best_i);
    if (lane == 0) out[1] = r4;
}

// ------------------------------------------------------------------ synthetic evaluator (tests)
__global__ __launch_bounds__(64) void k_synth_eval(SpParams p) {
    const int g = blockIdx.x, lane = threadIdx.x;
    GameCtl& c = p.ctl[g];
    if (c.status != ST_ACTIVE || c.leaf_kind != LK_EVAL) return;
    const Position& pos = p.tpos[(size_t)g * p.tpos_cap + c.n_exp];
    uint64_t h = synth_pos_hash(pos) ^ p.synth_salt;
    int n = c.n_legal;
    const uint16_t* lm = p.legal_mv + (size_t)g * MAXC;
    if (p.evaluator == SYNTH_UNIFORM) {
        // tie tests: every sibling has the same prior and every leaf the value 0, so all unvisited children of a node tie
        // exactly and find_max's LAST-maximum rule (src/mcts.rs:78-88) decides every descent
        for (int i = lane; i < n; i += 64) p.prior[(size_t)g * MAXC + i] = 1.0f / (float)n;
        if (lane == 0) p.value[g] = 0.0f;
        return;
    }
    // SYNTH_COARSE: 2-bit weights and values from {-0.5, 0, 0, 0.5}: exact PUCT ties between SOME siblings, next to
    // non-zero value sums (the hash evaluator's 24-bit priors never collide)
    const bool coarse = p.evaluator == SYNTH_COARSE;
    unsigned long long sum = 0;
    for (int i = lane; i < n; i += 64) sum += coarse ? 1u + (synth_weight(h, lm[i]) >> 22) : synth_weight(h, lm[i]);
    sum = scw::wave_sum_u64(sum);
    float fs = (float)sum;
    for (int i = lane; i < n; i += 64)
        p.prior[(size_t)g * MAXC + i] = (float)(coarse ? 1u + (synth_weight(h, lm[i]) >> 22) : synth_weight(h, lm[i])) / fs;
    if (lane == 0) {
        const float v = synth_value(h);
        p.value[g] = coarse ? (v < -0.5f ? -0.5f : v >= 0.5f ? 0.5f : 0.0f) : v;
    }
}

// ------------------------------------------------------------------ match play with slot recycling (sc_selfplay_set_match)
// Every live game of a fixed-rollout handle ends its ply in the same launch, t % rollout == 0, and launch t is evaluated by
// player (t / rollout) & 1 for ALL slots.  So games of different ages share a handle as long as each of them starts at such a
// boundary, in a launch its White evaluates: from then on its even plies fall on its White's launches.  The search kernels know
// nothing of this: the host gives them total_games = 0, so a slot whose game ends goes idle (start_new_game), and runs the two
// phases of k_match_boundary between the two halves of a boundary launch -- after the expansions that end the ply, before the
// selection of the next ply's first leaves.
// The player that is White in game ordinal k:
__device__ inline int match_white(const SpParams& p, unsigned long long k) { return p.match_colours ? (int)(k & 1) : 0; }
// The next ordinal whose White is player `side`, or total_games when there is none left.  One counter per side keeps the
// ordinals unique and every game 0..total_games-1 played once: with alternating colours side j draws j, j + 2, j + 4, ...
// (an odd total leaves the extra game to player 0), otherwise side 0 draws 0, 1, 2, ... and side 1 nothing.
__device__ inline unsigned long long match_ordinal(SpParams& p, int lane, int side) {
    const unsigned long long total = (unsigned long long)p.total_games;
    if (!p.match_colours && side) return total;
    unsigned long long n = 0;
    if (lane == 0) n = atomicAdd(&p.cnt->match_next[side], 1ULL);
    n = __shfl(n, 0, 64);
    const unsigned long long k = p.match_colours ? 2ULL * n + (unsigned long long)side : n;
    return k < total ? k : total;
}
// Opening lines (sc_selfplay_set_openings).  Game ordinal k plays line (colours ? k >> 1 : k) % n: with alternating colours the
// games 2j and 2j + 1 share a line, each player is White on it once.
__device__ inline int match_line_of(const SpParams& p, const MatchLines& ln, unsigned long long k) {
    return (int)((p.match_colours ? k >> 1 : k) % (unsigned long long)ln.n);
}
// A game that has just become ST_ACTIVE (try_start_game: start position, ply 0) moves to the end of its line: the line's L + 1
// records, replayed once by k_open_lines, become hist[0..L] of the slot, the last of them the root's position, and the search
// starts at ply L.  Plain vector loads and stores, 8 bytes a lane; L + 1 <= hist_cap is the host's check.
__device__ inline void match_copy_line(SpParams& p, int g, int lane, const Position* line, int len) {
    constexpr int W = (int)(sizeof(Position) / 8);
    static_assert(sizeof(Position) % 8 == 0, "a record is copied in 8-byte words");
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(line);
    unsigned long long* hist = reinterpret_cast<unsigned long long*>(p.hist + (size_t)g * p.hist_cap);
    unsigned long long* root = reinterpret_cast<unsigned long long*>(p.tpos + (size_t)g * p.tpos_cap);
    const int words = (len + 1) * W;
    wave_sync();   // (lane 0's stores of the start position, try_start_game, are complete before other lanes store to the same records)
    for (int i = lane; i < words; i += 64) hist[i] = src[i];
    if (lane < W) root[lane] = src[len * W + lane];
    if (lane == 0) {
        p.ctl[g].ply = len;
        p.ctl[g].start_ply = len;
    }
}
// Phase 1 for one slot.  A free slot takes a game that can start at THIS boundary if one is left, else one of the other side,
// which starts one ply later: while games remain a slot waits one ply at the most between two games (a busy trace-ring row
// aside).  A game that may not start yet parks its ordinal in the slot, as one that waits for a ring row does (try_start_game),
// but as ST_MATCH_WAIT: the search kernel retries ST_PENDING in every launch, and a match game must start at a boundary.
// With opening lines the first searched ply of game k, ply L of the game, is its White's only if L is even: the game starts at a
// boundary of player white(k) ^ (L & 1).  The ordinals are drawn as before -- the line, and with it the parity, is known only
// once the ordinal is -- and a game of the other parity waits its one ply.
__device__ inline void match_slot_start(SpParams& p, const MatchLines& ln, int g, int lane) {
    GameCtl& c = p.ctl[g];
    const int st = c.status, side = p.match_side & 1;
    const unsigned long long total = (unsigned long long)p.total_games;
    unsigned long long k;
    if (st == ST_MATCH_WAIT) {
        k = c.game_id - p.first_game_id;
    } else if (st == ST_IDLE) {
        k = match_ordinal(p, lane, side);
        if (k >= total) k = match_ordinal(p, lane, side ^ 1);
        if (k >= total) return;
    } else {
        return;
    }
    wave_sync();
    int len = 0;
    const Position* line = nullptr;
    if (ln.n > 0) {
        const int i = match_line_of(p, ln, k);
        const uint32_t a = ln.off[i], b = ln.off[i + 1];
        line = ln.tab + a;
        len = (int)(b - a) - 1;
    }
    if (side == (match_white(p, k) ^ (len & 1))) {
        try_start_game(p, g, lane, k);
        int now = 0;
        if (lane == 0) {
            now = c.status;
            if (now == ST_PENDING) c.status = ST_MATCH_WAIT;
        }
        if (len > 0 && __shfl(now, 0, 64) == ST_ACTIVE) match_copy_line(p, g, lane, line, len);
    } else if (lane == 0) {
        c.status = ST_MATCH_WAIT;
        c.leaf_kind = LK_NONE;
        c.game_id = p.first_game_id + k;
    }
}
// phase 0: a slot whose game has ended since the last boundary counts it -- int32 [slot][White's player][White won / Black won
// / draw / no outcome], the slot's own row -- from the game's trace header, which no later game can have taken yet: rows are
// taken in phase 1 only, a launch of its own.  trace_slot < 0 marks the slot as counted.  phase 1: match_slot_start.
__global__ __launch_bounds__(64) void k_match_boundary(SpParams p, MatchLines ln, int phase) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (phase == 1) {
        match_slot_start(p, ln, g, lane);
        return;
    }
    GameCtl& c = p.ctl[g];
    if (lane != 0 || c.status != ST_IDLE || c.trace_slot < 0) return;
    const TraceHdr& th = p.thdr[c.trace_slot];
    const int w = match_white(p, c.game_id - p.first_game_id);
    const int r = !th.has_outcome ? 3 : th.winner == 1 ? 0 : th.winner == 0 ? 1 : 2;
    p.match_tally()[((size_t)g * 2 + w) * 4 + r] += 1;
    c.trace_slot = -1;
}

__global__ __launch_bounds__(64) void k_init_slots(SpParams p, MatchLines ln) {
    const int g = blockIdx.x, lane = threadIdx.x;
    uint4* b = reinterpret_cast<uint4*>(p.boards + (size_t)g * 7168);
    for (int i = lane; i < 448; i += 64) b[i] = make_uint4(0, 0, 0, 0);
    if (lane < 8) p.meta[(size_t)g * 8 + lane] = 0;
    if (lane == 0) p.n_legal[g] = 0;
    if (p.match_recycle) {
        // (sc_selfplay_set_match runs this kernel again on the handle's fresh state, and sc_selfplay_set_openings once more, with
        // the lines.)  This is the boundary of ply 0, player 0's: a slot takes a game with player 0 as White, which starts now, or
        // one of player 1's and waits a ply
        if (lane == 0) {
            p.ctl[g].status = ST_IDLE;
            p.ctl[g].leaf_kind = LK_NONE;
            p.ctl[g].trace_slot = -1;
        }
        wave_sync();
        match_slot_start(p, ln, g, lane);
        return;
    }
    // slot g starts with game g (a deterministic slot <-> game map at start; later games are drawn from the counter as
    // slots free up); no game has finished yet, so nothing else touches the counter during this launch
    if (g == 0 && lane == 0)
        atomicAdd(&p.cnt->next_game, (unsigned long long)(p.n_slots < p.total_games ? p.n_slots : p.total_games));
    if (g >= p.total_games) {
        if (lane == 0) {
            p.ctl[g].status = ST_IDLE;
            p.ctl[g].leaf_kind = LK_NONE;
        }
        return;
    }
    try_start_game(p, g, lane, (unsigned long long)g);
}

// One wave per case (test aid, sc_debug_choose_child): case c reads n_act[c][0..nc[c]), temperature[c], u[c] and the weight
// table of its temperature, w[w_off[c] .. + w_max].
__global__ __launch_bounds__(64) void k_debug_choose_child(int n_cases, const int32_t* n_act, const int32_t* nc, const float* temperature,
                                                           const float* u, int tie_random, const float* w, const int32_t* w_off, int w_max,
                                                           int32_t* choice, float* total) {
    const int c = blockIdx.x, lane = threadIdx.x;
    if (c >= n_cases) return;
    float tot;
    const int ch = choose_child(n_act + (size_t)c * MAXC, uniform(nc[c]), temperature[c], u[c], tie_random, lane, w + uniform(w_off[c]), w_max, &tot);
    if (lane == 0) {
        choice[c] = ch;
        total[c] = tot;
    }
}

// One launch per simulation step: finish the previous simulation of every game (value head tail, expand,
// backward, and at the end of a ply mcts::step + trace + outcome), then select the next leaf and encode it.
__global__ __launch_bounds__(64) void k_mcts(SpParams p, int do_expand, int do_select) {
    const int g = blockIdx.x, lane = threadIdx.x;
    __shared__ __attribute__((aligned(16))) int8_t s_stage[7168];
    __shared__ move_t s_moves[MAXC];
    __shared__ Position s_pos;
    __shared__ Position s_hist[8];
    __shared__ uint16_t s_ps[DEPTH_LDS];
    constexpr bool SC_ST = true;   // (k_mcts runs the flush, the timed samples and the synthetic evaluators: never the hot loop)
    SC_STAMP(0);
    GameCtl cs_pre{};
    bool cs_pre_valid = false;
    if (do_expand) {
        // No fence between the two halves: the block is ONE wavefront, whose vector-memory operations reach the cache
        // hierarchy in program order, so the selection below reads what the expansion above stored (statistics of the
        // path, control block, tree headers) without first waiting for every store to be acknowledged (~4 k cycles).
        dev_expand(p, g, lane, &s_pos, cs_pre, cs_pre_valid);
        __builtin_amdgcn_wave_barrier();
    }
    SC_STAMP(1);
    if (do_select) dev_select(p, g, lane, s_stage, s_moves, &s_pos, s_ps, s_hist, cs_pre, cs_pre_valid);
}

// ------------------------------------------------------------------ sc_selfplay_match_tally
// out[w * 4 + r] = the sum over the slots of tally[slot][w][r] (k_match_boundary); one wave, thread = column
__global__ __launch_bounds__(64) void k_match_tally(const int32_t* tally, int n_slots, long long* out) {
    const int j = threadIdx.x;
    if (j >= 8) return;
    long long s = 0;
    for (int g = 0; g < n_slots; g++) s += tally[(size_t)g * 8 + j];
    out[j] = s;
}

// ------------------------------------------------------------------ sc_selfplay_set_openings
// One wave per line, once per handle: replay line i from the start position into its records tab[rec_off[i] ..], as k_set_position
// replays a slot's move list into its chain (the same replay_step: keys, repetition and irreversibility flags), with every move
// checked against the generated legal moves.  status[i]: 0 ok; -(j + 1): move j is not legal; 1: the game is over in the line's
// last position (outcome(claim_draw=True), or no legal move).  rec_off[i + 1] - rec_off[i] = the line's length + 1: the host's sum.
// With bases (sc_selfplay_set_openings_from) line i starts from its base where it has one (chain_start).  The host may leave room for `pad` records in front of it (rec_off[i + 1] - rec_off[i] = pad + length + 1): they
// are written empty -- no men, no flags: zero planes for the encoder -- and the base then carries F_IRREV, so that no repetition
// scan of the game walks past it into them (a scan from the start of a chain stops at index 0 by itself).
__global__ __launch_bounds__(64) void k_open_lines(int n_lines, const uint16_t* moves, const uint32_t* move_off, Position* tab,
                                                   const uint32_t* rec_off, int32_t* status, Bases bases) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n_lines) return;
    __shared__ move_t s_moves[MAXC];
    __shared__ Position s_np;
    const uint16_t* mv = moves + move_off[i];
    const int nm = (int)(move_off[i + 1] - move_off[i]);
    const int pad = (int)(rec_off[i + 1] - rec_off[i]) - 1 - nm;
    Position* hist = tab + rec_off[i] + (pad > 0 ? pad : 0);
    Position cur = chain_start(bases, i, true);
    if (lane == 0) {
        Position none;
        set_startpos(none);
#pragma unroll
        for (int t = 0; t < 6; t++) none.pcs[t] = 0;
        none.occ[0] = none.occ[1] = 0;
        none.castling = 0;
        for (int k = 0; k < pad; k++) tab[rec_off[i] + k] = none;
        hist[0] = cur;
    }
    __syncthreads();
    int st;
    replay_checked(cur, mv, nm, hist, s_moves, &s_np, lane, st);
    if (st == 0) {
        int n = 0, winner = -1;
        gen_legal_wave(cur, s_moves, lane, n);
        __syncthreads();
        const HistChain hc{hist};
        if (outcome_claim_draw(hc, nm, &winner) != T_NONE || n == 0) st = 1;
    }
    if (lane == 0 && pad > 0) hist[0].flags = F_IRREV;   // (after the scans above, which start at the base anyway)
    if (lane == 0) status[i] = st;
}

// ------------------------------------------------------------------ sc_selfplay_set_position
// base (or null: the start position): a validated record of fen_kernels.hip, hist[0] of the slot
__global__ __launch_bounds__(64) void k_set_position(SpParams p, int g, const uint16_t* moves, int n_moves, const Position* base) {
    const int lane = threadIdx.x;
    GameCtl& c = p.ctl[g];
    Position* hist = p.hist + (size_t)g * p.hist_cap;
    Position* tpos = p.tpos + (size_t)g * p.tpos_cap;
    __shared__ Position s_np;
    Position cur;
    if (base) {
        cur = uniform(*base);
    } else {
        set_startpos(cur);
        cur.key = position_key(cur);
    }
    if (lane == 0) hist[0] = cur;
    __syncthreads();
    for (int i = 0; i < n_moves && i + 1 < p.hist_cap; i++) replay_step(cur, moves[i], i, hist, tpos, &s_np, lane);
    if (lane == 0) {
        const size_t nb = (size_t)g * p.node_cap;
        tpos[0] = cur;
        p.N[nb] = 0;
        p.W[nb] = 0.0f;
        p.H[nb] = NodeHdr{-1, 0, 0};
        c.ply = n_moves;
        c.start_ply = n_moves;
        c.sim = 0;
        c.n_nodes = 1;
        c.n_exp = 1;
        c.leaf_kind = LK_NONE;
        c.rollout_cur = p.rollout;
        c.status = ST_ACTIVE;
    }
}

}  // namespace sc

namespace scl {
void init_slots(const sc::SpParams& p, const sc::MatchLines& lines, hipStream_t s) {
    hipLaunchKernelGGL(sc::k_init_slots, dim3(p.n_slots), dim3(64), 0, s, p, lines);
}
void mcts(const sc::SpParams& p, int do_expand, int do_select, hipStream_t s) {
    hipLaunchKernelGGL(sc::k_mcts, dim3(p.n_slots), dim3(64), 0, s, p, do_expand, do_select);
}
void synth_eval(const sc::SpParams& p, hipStream_t s) { hipLaunchKernelGGL(sc::k_synth_eval, dim3(p.n_slots), dim3(64), 0, s, p); }
void debug_find_max(const float* d_u, int n, int* d_out, hipStream_t s) { hipLaunchKernelGGL(sc::k_debug_find_max, dim3(1), dim3(64), 0, s, d_u, n, d_out); }
void debug_choose_child(int n_cases, const int32_t* d_n_act, const int32_t* d_nc, const float* d_temperature, const float* d_u, int tie_random,
                        const float* d_w, const int32_t* d_w_off, int w_max, int32_t* d_choice, float* d_total, hipStream_t s) {
    if (n_cases <= 0) return;
    hipLaunchKernelGGL(sc::k_debug_choose_child, dim3(n_cases), dim3(64), 0, s, n_cases, d_n_act, d_nc, d_temperature, d_u, tie_random,
                       d_w, d_w_off, w_max, d_choice, d_total);
}
void match_boundary(const sc::SpParams& p, const sc::MatchLines& lines, hipStream_t s) {
    hipLaunchKernelGGL(sc::k_match_boundary, dim3(p.n_slots), dim3(64), 0, s, p, lines, 0);
    hipLaunchKernelGGL(sc::k_match_boundary, dim3(p.n_slots), dim3(64), 0, s, p, lines, 1);
}
void open_lines(int n_lines, const uint16_t* d_moves, const uint32_t* d_move_off, sc::Position* d_tab, const uint32_t* d_rec_off,
                int32_t* d_status, const sc::Bases& bases, hipStream_t s) {
    if (n_lines <= 0) return;
    hipLaunchKernelGGL(sc::k_open_lines, dim3(n_lines), dim3(64), 0, s, n_lines, d_moves, d_move_off, d_tab, d_rec_off, d_status, bases);
}
void match_tally(const int32_t* d_tally, int n_slots, long long* d_out, hipStream_t s) {
    hipLaunchKernelGGL(sc::k_match_tally, dim3(1), dim3(64), 0, s, d_tally, n_slots, d_out);
}
void set_position(const sc::SpParams& p, int slot, const uint16_t* d_moves, int n_moves, hipStream_t s, const sc::Position* d_base) {
    hipLaunchKernelGGL(sc::k_set_position, dim3(1), dim3(64), 0, s, p, slot, d_moves, n_moves, d_base);
}
}  // namespace scl
