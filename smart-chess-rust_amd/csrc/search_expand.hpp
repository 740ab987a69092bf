// search_expand.hpp -- the other half of a simulation step: game start and finish, the end-of-ply move choice, the value
// tail's loads and dev_expand (expand, backward, mcts::step).  Device functions only; contraction: see search_select.hpp.
#pragma once
#include "search_select.hpp"
#include "value_tail.hpp"

namespace sc {
// ------------------------------------------------------------------ game (re)start
// Game ordinal k (0-based on this handle) takes trace-ring row k % trace_cap, strictly after game k - trace_cap: the row
// must hold THAT game, finished (and, with trace_hold, released by the host: sc_selfplay_poll).  A long game next to slots
// that cycle through short ones can be lapped -- writing its rows would corrupt both traces -- and several waiting games
// can map to the same row (k + cap, k + 2 cap, ...): they start one after the other.  A slot that cannot start parks its
// ordinal in game_id (ST_PENDING) and retries at every simulation step.
__device__ inline void try_start_game(SpParams& p, int g, int lane, unsigned long long k) {
    GameCtl& c = p.ctl[g];
    const int ts = (int)(k % (unsigned long long)p.trace_cap);
    const int st = p.thdr[ts].state;
    const unsigned long long prev_id = p.thdr[ts].game_id;
    bool ok;
    if (k < (unsigned long long)p.trace_cap) ok = st == TR_FREE;   // first use of the row
    else ok = prev_id == p.first_game_id + k - (unsigned long long)p.trace_cap && (st == TR_FREE || (st == TR_DONE && !p.trace_hold));
    if (!ok) {
        if (lane == 0) {
            c.status = ST_PENDING;
            c.leaf_kind = LK_NONE;
            c.game_id = p.first_game_id + k;
        }
        return;
    }
    const size_t nb = (size_t)g * p.node_cap;
    if (lane == 0) {
        Position s;
        set_startpos(s);
        s.key = position_key(s);
        p.hist[(size_t)g * p.hist_cap] = s;
        p.tpos[(size_t)g * p.tpos_cap] = s;
        p.N[nb] = 0;
        p.W[nb] = 0.0f;
        p.P[nb] = 0.0f;
        p.U[nb] = 0.0f;
        p.MV[nb] = 0;
        p.H[nb] = NodeHdr{-1, 0, 0};
        c.status = ST_ACTIVE;
        c.ply = 0;
        c.start_ply = 0;
        c.sim = 0;
        c.n_nodes = 1;
        c.n_exp = 1;
        c.leaf = 0;
        c.path_len = 0;
        c.leaf_kind = LK_NONE;
        c.n_legal = 0;
        c.err = 0;
        c.rollout_cur = p.rollout;
        c.game_id = p.first_game_id + k;
        c.trace_slot = ts;
        TraceHdr& th = p.thdr[ts];
        th.n_steps = 0;
        th.has_outcome = 0;
        th.termination = 0;
        th.winner = -1;
        th.game_id = c.game_id;
        th.state = TR_LIVE;
    }
}
__device__ inline void start_new_game(SpParams& p, int g, int lane) {
    GameCtl& c = p.ctl[g];
    unsigned long long k = 0;
    if (lane == 0) k = atomicAdd(&p.cnt->next_game, 1ULL);
    k = __shfl(k, 0, 64);
    if (k >= (unsigned long long)p.total_games) {
        if (lane == 0) {
            c.status = ST_IDLE;
            c.leaf_kind = LK_NONE;
        }
        return;
    }
    try_start_game(p, g, lane, k);
}

__device__ inline void finish_game(SpParams& p, int g, int lane, int has_outcome, int term, int winner) {
    GameCtl& c = p.ctl[g];
    if (lane == 0) {
        TraceHdr& th = p.thdr[c.trace_slot];
        th.n_steps = c.ply - c.start_ply;
        th.has_outcome = has_outcome;
        th.termination = term;
        th.winner = winner;
        th.game_id = c.game_id;
        __threadfence();
        th.state = TR_DONE;
        atomicAdd(&p.cnt->games_finished, 1);
        c.status = ST_FINISHED;
    }
    wave_sync();
    start_new_game(p, g, lane);
}

// ------------------------------------------------------------------ the end-of-ply move choice
// mcts::step (mcts.rs:298-317) on the visit counts n_act[0..nc) of the root's children (nc >= 1), called by the whole wave with
// wave-uniform arguments: `temperature` already resolved for the ply, u in [0,1) the ply's uniform draw.  Returns the chosen
// child; *total = the f32 sum of the weights of the weighted branch (0 at temperature 0).  The one implementation: the
// self-play kernels and the test aid k_debug_choose_child (sc_debug_choose_child) both call it.
// The weight N^(1/temperature) is READ from w[0..w_max], which the host filled with ITS libm's powf for this temperature
// (host_common.hpp choice_weights): the reference's f32::powf is that function, and the index below must be the reference's bit for
// bit -- the device's own powf is one ulp off it for a quarter of all (count, temperature) pairs.  Temperature 1
// (the temperature-switch window) needs no table: powf(n, 1) == n.  A count never exceeds the ply's simulation budget, which
// the table covers; the index is clamped all the same so that no read can leave the table.
__device__ inline int choose_child(const int32_t* n_act, int nc, float temperature, float u, int tie_random, int lane, const float* w,
                                   int w_max, float* total) {
    *total = 0.0f;
    if (temperature == 0.0f) {
        int bn = -1, bi = 0x7fffffff;
        for (int i = lane; i < nc; i += 64) {
            int n = n_act[i];
            if (n > bn) {  // first maximum within the lane (indices increase)
                bn = n;
                bi = i;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            int on = __shfl_xor(bn, o, 64), oi = __shfl_xor(bi, o, 64);
            if (on > bn || (on == bn && oi < bi)) {
                bn = on;
                bi = oi;
            }
        }
        int choice = bi;
        if (tie_random) {
            // NNPlayer::bestmove (play.rs:268-277): uniform among the maxima; k = floor(u * count), in index order
            int cnt = 0;
            for (int i = 0; i < nc; i++) cnt += n_act[i] == bn;
            int k = (int)(u * (float)cnt);
            if (k >= cnt) k = cnt - 1;
            for (int i = 0; i < nc; i++)
                if (n_act[i] == bn && k-- == 0) {
                    choice = i;
                    break;
                }
        }
        return choice;
    }
    // WeightedIndex over N^(1/temp): sequential f32 cumulative sums, x = u*total,
    // index = number of cumulative weights (last excluded) <= x
    const bool plain = 1.0f / temperature == 1.0f;
    auto weight = [&](int n) { return plain ? (float)n : w[n < w_max ? n : w_max]; };
    float sum = 0.0f;
    for (int i = 0; i < nc; i++) sum += weight(n_act[i]);
    *total = sum;
    float x = u * sum;
    float cum = 0.0f;
    int idx = 0;
    for (int i = 0; i < nc - 1; i++) {
        cum += weight(n_act[i]);
        if (cum <= x) idx++;
    }
    return idx;
}

// ------------------------------------------------------------------ expand + backward + mcts::step
// mcts.rs:267-288 (expand, backward), then when the rollout count is reached the per-ply part of
// src/main.rs:198-233: snapshot root/children into the trace, mcts::step (mcts.rs:292-328), outcome.
// value head tail for one position (nn_kernels.hip k_value_finish, fused here so that the search step needs
// no separate launch): + meta columns + bias, ReLU, Linear 128->1, tanh, times (2*turn-1)
// Two halves: every address depends on the game slot only, so the loads are requested at the very top of the expansion,
// together with the control block (one round trip earlier than the path statistics, which need the control block).
using scvt::ValueTail;
__device__ __forceinline__ void value_tail_issue(const SpParams& p, int g, int lane, ValueTail& t) {
    const float* wf = p.vf_w;
    const int32_t* meta = p.meta + (size_t)g * 8;
#pragma unroll
    for (int k = 0; k < 7; k++) t.meta[k] = meta[k];
    // lane owns output columns 2*lane, 2*lane+1; ALL split-K partials are requested before the first add (one L2
    // round trip instead of one per 32 partials), then summed in fixed ascending order by value_tail.hpp's
    // value_tail_compute -- the function k_value_finish calls too (tests/test_gpu_netloop.py: bitwise identical)
    const int j = 2 * lane;
    const float* vp = p.vpart + (size_t)g * 128 + j;
    const size_t vstride = (size_t)p.n_slots * 128;
    // split-K is 32 or 64 (host_common.hpp): two unconditional batches -- a per-partial bound check makes the compiler
    // branch around (and wait for) every single load
#pragma unroll
    for (int ks = 0; ks < 32; ks++) t.acc[ks] = *reinterpret_cast<const float2*>(vp + (size_t)ks * vstride);
    if (p.vf_ksplit > 32) {
#pragma unroll
        for (int ks = 32; ks < 64; ks++) t.acc[ks] = *reinterpret_cast<const float2*>(vp + (size_t)ks * vstride);
    } else {
#pragma unroll
        for (int ks = 32; ks < 64; ks++) t.acc[ks] = make_float2(0.f, 0.f);
    }
    t.bias = *reinterpret_cast<const float2*>(wf + p.vf_fc1b + j);
    t.w2 = *reinterpret_cast<const float2*>(wf + p.vf_fc2w + j);
#pragma unroll
    for (int k = 0; k < 7; k++) t.wm[k] = *reinterpret_cast<const float2*>(wf + p.vf_fc1m + k * 128 + j);
    t.fc2b = wf[p.vf_fc2b];
}
__device__ __forceinline__ float value_tail_finish(const SpParams& p, const ValueTail& t) { return scvt::value_tail_compute(t, p.vf_ksplit); }

// cs_out / cs_valid: the control block as this function leaves it, handed to dev_select in registers (a reload would be
// a load of words stored a few instructions earlier); not valid after a ply transition
template <bool SC_ST = true>
__device__ __forceinline__ void dev_expand(SpParams& p, int g, int lane, Position* s_np_p, GameCtl& cs_out, bool& cs_valid) {
#pragma clang fp contract(off)
    Position& s_np = *s_np_p;
    GameCtl& c = p.ctl[g];
    // First round trip: EVERYTHING whose address depends on the game slot only -- the control block (one 64-byte
    // fetch), the recorded path, the leaf's priors and legal moves, the slot counters, the value partials.  Order
    // matters: the loads are issued with clamped indices and no guards, and the control block is moved to SGPRs only
    // AFTER the last of them -- a readfirstlane right behind its load (or a load under `cond ? load : 0`, which becomes
    // a branch around the load with its own wait) parks the wave for a full round trip before the next load is even
    // issued: the kernel used to start with three serialised trips (control block, path, the rest).
    // ... and the kernel arguments those addresses are made of are fetched TOGETHER: left to itself the compiler reads each of
    // them (scattered over the argument block's cache lines) where it is first used, behind a wait of its own -- 3 k cycles
    // passed between the entry of this function and the issue of its last load (tools/dbg_expand.py).  The empty asm statement
    // wants them all in SGPRs at one point: one batch of scalar loads, one wait.
    {
        const void *a0 = p.ctl, *a1 = p.path, *a2 = p.prior, *a3 = p.legal_mv, *a4 = p.slot_cnt, *a5 = p.vpart, *a6 = p.vf_w, *a7 = p.meta;
        const int i0 = p.max_depth, i1 = p.vf_fused, i2 = p.n_slots, i3 = p.vf_ksplit;
        const uint32_t u0 = p.vf_fc1b, u1 = p.vf_fc1m, u2 = p.vf_fc2w, u3 = p.vf_fc2b;
        asm volatile("" ::"s"(a0), "s"(a1), "s"(a2), "s"(a3), "s"(a4), "s"(a5), "s"(a6), "s"(a7), "s"(i0), "s"(i1), "s"(i2), "s"(i3), "s"(u0), "s"(u1),
                     "s"(u2), "s"(u3));
    }
    const GameCtl craw = c;
    const int pth_raw = p.path[(size_t)g * p.max_depth + (lane < p.max_depth ? lane : p.max_depth - 1)];
    float prv[4];
    uint16_t lmv[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int i = lane + 64 * k, ic = i < MAXC ? i : MAXC - 1;
        prv[k] = p.prior[(size_t)g * MAXC + ic];
        lmv[k] = p.legal_mv[(size_t)g * MAXC + ic];
    }
    const unsigned long long sc_sims = p.slot_cnt[(size_t)g * 2], sc_evals = p.slot_cnt[(size_t)g * 2 + 1];
    ValueTail vt;
    if (p.vf_fused) value_tail_issue(p, g, lane, vt);   // used when the leaf turns out to be a network evaluation
    __builtin_amdgcn_sched_barrier(0);
    const GameCtl cs = uniform(craw);
    const int pth = lane < p.max_depth ? pth_raw : 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int i = lane + 64 * k;
        prv[k] = i < MAXC ? prv[k] : 0.f;
        lmv[k] = i < MAXC ? lmv[k] : (uint16_t)0;
    }
    cs_out = cs;
    cs_valid = true;
    if (cs.status == ST_PENDING) {   // waiting for its trace-ring row (try_start_game)
        try_start_game(p, g, lane, cs.game_id - p.first_game_id);
        cs_valid = false;
        return;
    }
    if (cs.status != ST_ACTIVE || cs.leaf_kind == LK_NONE) return;
    const size_t nb = (size_t)g * p.node_cap;
    int32_t* N = p.N + nb;
    float* W = p.W + nb;
    float* P = p.P + nb;
    float* U = p.U + nb;
    uint16_t* MV = p.MV + nb;
    NodeHdr* H = p.H + nb;
    const int32_t* path = p.path + (size_t)g * p.max_depth;
    Position* hist = p.hist + (size_t)g * p.hist_cap;
    Position* tpos = p.tpos + (size_t)g * p.tpos_cap;

    const int leaf = cs.leaf, kind = cs.leaf_kind, plen = cs.path_len;
    float value = cs.leaf_value;
    int n_nodes = cs.n_nodes, n_exp = cs.n_exp;
    uint32_t err = 0;
    // Everything whose address depends on the game only (the recorded path, the leaf's priors and legal moves) was
    // requested together with the control block above; the statistics of the path nodes are requested now, before
    // the value tail, so the whole expansion costs two L2 round trips instead of five dependent ones.
    const bool inpath = lane < plen;
    int n0 = 0;
    float w0 = 0.f;
    if (inpath) {
        n0 = N[pth];
        w0 = W[pth];
    }
    if (kind == LK_EVAL) {
        value = p.vf_fused ? value_tail_finish(p, vt) : p.value[g];
        int n = cs.n_legal;
        if (n_nodes + n > p.node_cap || n_exp + 1 >= p.tpos_cap) {
            err = ERR_POOL_OVERFLOW;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                int i = lane + 64 * k;
                if (i < n) {
                    int id = n_nodes + i;
                    N[id] = 0;
                    W[id] = 0.0f;
                    P[id] = prv[k];
                    U[id] = 0.0f;
                    MV[id] = lmv[k];
                    H[id] = NodeHdr{-1, 0, 0};
                }
            }
            if (lane == 0) H[leaf] = NodeHdr{n_nodes, (uint16_t)n, (uint16_t)n_exp};
            n_nodes += n;
            n_exp += 1;
        }
    } else if (kind == LK_TERM_NEW) {
        if (lane == 0) H[leaf] = NodeHdr{value == 0.0f ? -2 : value > 0.0f ? -3 : -4, 0, 0};
    }
    // backward (mcts.rs:90-98): every node of the path, root included
    if (inpath) {
        N[pth] = n0 + 1;
        W[pth] = w0 + value;
    }
    for (int d = lane + 64; d < plen; d += 64) {
        int nd = path[d];
        N[nd] += 1;
        W[nd] += value;
    }
    wave_sync();
    int sim = cs.sim + 1;
    if (lane == 0) {
        c.n_nodes = n_nodes;
        c.n_exp = n_exp;
        c.sim = sim;
        c.leaf_kind = LK_NONE;
        if (err) {
            c.err = cs.err | err;
            atomicOr(&p.cnt->err, (int)err);
        }
        // per-slot counters (summed by the host): 256 waves adding to ONE global counter at the same moment serialise
        // in the L2 atomic unit, and this wave's next loads queue behind its own atomics (in-order vmcnt)
        p.slot_cnt[(size_t)g * 2] = sc_sims + 1ULL;
        if (kind == LK_EVAL) p.slot_cnt[(size_t)g * 2 + 1] = sc_evals + 1ULL;
    }
    cs_out.n_nodes = n_nodes;
    cs_out.n_exp = n_exp;
    cs_out.sim = sim;
    cs_out.leaf_kind = LK_NONE;
    cs_out.err = cs.err | err;
    const int budget = p.rollout_factor > 0.f ? cs.rollout_cur : p.rollout;
    if (sim < budget) return;
    cs_valid = false;

    // ---------------- end of this ply's search (main.rs:198-233)
    wave_sync();
    const int ply = cs.ply;
    const NodeHdr h0 = H[0];
    const int nc = h0.nc, fc = h0.fc;
    if (nc == 0 || budget == 0) {
        // mcts::step -> None: no children => no legal moves (main.rs:213-216), or a --rollout-factor budget of 0
        // simulations (the reference then searches nothing and the root stays childless)
        HistChain hc{hist};
        int winner = -1;
        int term = outcome_claim_draw(hc, ply, &winner);
        finish_game(p, g, lane, term != T_NONE, term, winner);
        return;
    }
    const int ts = cs.trace_slot;
    const size_t tstep = (size_t)ts * p.num_steps + (size_t)(ply - cs.start_ply);
    for (int i = lane; i < nc; i += 64) {
        p.t_cmove[tstep * MAXC + i] = MV[fc + i];
        p.t_cn[tstep * MAXC + i] = N[fc + i];
        p.t_cq[tstep * MAXC + i] = W[fc + i];
        p.t_cu[tstep * MAXC + i] = U[fc + i];
    }
    // mcts::step (mcts.rs:298-317)
    const float temperature = (ply - cs.start_ply) < p.temp_switch ? 1.0f : p.temperature;
    const float u = (float)(sc_rng(p.seed, cs.game_id, (uint64_t)ply, 1, 0) >> 40) / 16777216.0f;
    float w_total;
    const int choice = choose_child(N + fc, nc, temperature, u, p.tie_random, lane, p.choice_w, p.choice_w_max, &w_total);
    move_t mv = MV[fc + choice];
    if (lane == 0) {
        p.t_move[tstep] = mv;
        p.t_q[tstep] = W[0];
        p.t_nchild[tstep] = nc;
    }
    // advance the game line
    Position np = uniform(hist[ply]);
    make_move(np, (move_t)uniform((int)mv));
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
    const int i_step = ply - cs.start_ply;  // the reference's loop index i
    if (i_step > p.outcome_gate) {         // main.rs:223-228
        HistChain hc{hist};
        int winner = -1;
        int term = outcome_claim_draw(hc, new_ply, &winner);
        if (term != T_NONE) {
            wave_sync();
            finish_game(p, g, lane, 1, term, winner);
            return;
        }
    }
    if (i_step + 1 >= p.num_steps || new_ply + 1 >= p.hist_cap) {  // loop ends: outcome stays null
        wave_sync();
        finish_game(p, g, lane, 0, 0, -1);
        return;
    }
    // fresh search tree rooted at the new position (chosen child is reset(), mcts.rs:319-323)
    if (lane == 0) {
        tpos[0] = np;
        N[0] = 0;
        W[0] = 0.0f;
        P[0] = 0.0f;
        U[0] = 0.0f;
        MV[0] = mv;
        H[0] = NodeHdr{-1, 0, 0};
        c.n_nodes = 1;
        c.n_exp = 1;
        c.sim = 0;
    }
}

}  // namespace sc
