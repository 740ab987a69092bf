// advance_kernels.hip -- sc_selfplay_advance: a move is played in a slot and the searched subtree below it is KEPT; the chosen
// root child becomes the root (mcts::step without the reset of mcts.rs:319-323).  One workgroup of 256 threads per listed slot.
//
// The tree lets this be one ascending sweep.  A node's child block is allocated after the node's own sibling block, so H[i].fc > i
// for every expanded node: marking [fc, fc + nc) for every marked, expanded i in ascending order of i finds the whole subtree of
// the child c.  The STABLE compaction -- a kept node's new index is the number of kept nodes with a smaller old index -- maps c to
// 0 and c's block to 1..nc, and because allocation order is expansion order the result is array for array the tree of a fresh
// search from the position after the move after N[c] simulations (tests/advance_ref.py holds that to the oracle).  New index <=
// old index holds for the stable order only, which is what allows the move IN PLACE: chunks are taken in ascending order and a
// chunk is read whole before it is written.  tpos records move the same way, in ascending order of their slot `ps`.
//
//   phase A  checks; the move is looked up among the root's children (or, root unexpanded, among the generated legal moves)
//   phase B  the sweep over [c, n_nodes), 256 nodes per chunk: a chunk is iterated until no thread has marked a block that starts
//            inside it (the worst case is a chain of one-child nodes: one iteration per node), then numbered -- wave_excl_scan_u32 per wave,
//            the four wave totals in LDS, and the running carry in a register of every thread: the scan lives inside this
//            workgroup's sweep, the only consumer that cannot use scl::exclusive_scan_u32 (the marks of a chunk depend on the
//            marks of the chunks before it).  The kept tpos slots are collected as a bitmap in LDS (ps is 16 bits: 8 KB); new ps =
//            1 + the set bits below it.  Every header is checked against the bounds the later phases index with.  Until here
//            nothing of the slot has been written: a refused entry changes nothing but its status.
//   phase C  wave 0: the trace step and the game line, the end-of-ply code of dev_expand (search_expand.hpp) statement for
//            statement with the pushed move in place of the chosen one
//   phase D  nodes, then tpos records, moved in place; the control block
//
// Scratch (AdvanceArgs::scratch): 4 B per LIVE node of the listed slots -- 0, or 1 + the new index.  Built with -ffp-contract=off
// as every unit that includes the search headers.
#include "search_expand.hpp"

#include "launchers.hpp"

namespace sc {
using scad::ADV_THREADS;
using scad::PS_WORDS;

// marks are written by one thread and read by another of the same workgroup, a barrier in between: relaxed atomics keep the
// compiler from holding them in registers, the barrier's fences order them
__device__ __forceinline__ uint32_t mark_load(const uint32_t* m) { return __hip_atomic_load(m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void mark_store(uint32_t* m, uint32_t v) { __hip_atomic_store(m, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// the exclusive prefix of v over the workgroup's threads and the total (every thread calls; two barriers)
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* s_wsum, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t wtot;
    const uint32_t pre = scw::wave_excl_scan_u32(v, &wtot);
    if (lane == 0) s_wsum[wave] = wtot;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < ADV_THREADS / 64; w++) {
        const uint32_t x = s_wsum[w];
        base += w < wave ? x : 0u;
        tot += x;
    }
    __syncthreads();
    *total = tot;
    return base + pre;
}

// Has any thread of the workgroup v?  One barrier per call: call k raises s_flag[k % 3] and thread 0 clears the flag of call k + 1,
// which the readers of call k - 2 have left behind call k - 1's barrier.  s_flag[0..3) starts at 0, k at 0 in every thread.
__device__ __forceinline__ bool block_any(bool v, int* s_flag, int& k) {
    if (threadIdx.x == 0) s_flag[(k + 1) % 3] = 0;
    if (v) s_flag[k % 3] = 1;
    __syncthreads();
    const bool r = s_flag[k % 3] != 0;
    k++;
    return r;
}

__global__ __launch_bounds__(ADV_THREADS) void k_advance(SpParams p, scad::AdvanceArgs a) {
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (e >= a.n) return;
    __shared__ move_t s_moves[MAXC];
    __shared__ Position s_np;
    __shared__ uint32_t s_ps[PS_WORDS];    // bit ps: an expanded node with that tpos slot is kept
    __shared__ uint32_t s_pre[PS_WORDS];   // the set bits below word w
    __shared__ uint32_t s_wsum[ADV_THREADS / 64];
    __shared__ uint32_t s_nexp;            // kept expanded nodes, counted node by node (against the bitmap's total)
    __shared__ int s_act, s_child, s_flag[3];
    int any_k = 0;

    // ------------------------------------------------------------ phase A (every thread reads the same words: block-uniform)
    auto refuse = [&](int st) {
        if (tid == 0) {
            a.status[e] = st;
            if (a.kept) a.kept[e * 3] = a.kept[e * 3 + 1] = a.kept[e * 3 + 2] = 0;
        }
    };
    const int g = uniform(a.slots[e]);
    if (g < 0 || g >= p.n_slots) {   // (the host has refused these already)
        refuse(-2);
        return;
    }
    GameCtl& c = p.ctl[g];
    const GameCtl cs = uniform(c);
    const size_t nb = (size_t)g * p.node_cap;
    int32_t* N = p.N + nb;
    float* W = p.W + nb;
    float* P = p.P + nb;
    float* U = p.U + nb;
    uint16_t* MV = p.MV + nb;
    NodeHdr* H = p.H + nb;
    Position* hist = p.hist + (size_t)g * p.hist_cap;
    Position* tpos = p.tpos + (size_t)g * p.tpos_cap;
    const uint64_t off0 = a.off[e], off1 = a.off[e + 1];
    uint32_t* M = a.scratch + off0;
    const int ply = cs.ply, i_step = cs.ply - cs.start_ply, ts = cs.trace_slot, n = cs.n_nodes, n_exp_old = cs.n_exp;
    bool ok = cs.status == ST_ACTIVE && cs.leaf_kind == LK_NONE;
    ok = ok && ply >= 0 && ply + 1 < p.hist_cap && i_step >= 0 && i_step < p.num_steps && ts >= 0 && ts < p.trace_cap;   // (what the stores below index)
    ok = ok && n >= 1 && n <= p.node_cap && (uint64_t)n <= off1 - off0 && n_exp_old >= 1 && n_exp_old <= p.tpos_cap;
    NodeHdr h0{-1, 0, 0};
    if (ok) {
        h0 = uniform(H[0]);
        if (h0.fc >= 0 && (h0.fc < 1 || h0.nc > MAXC || h0.fc + (int)h0.nc > n)) ok = false;
    }
    if (!ok) {
        refuse(-2);
        return;
    }
    const move_t mv = (move_t)uniform((int)a.moves[e]);
    const bool fresh_root = h0.fc == -1;
    int nl = 0;
    if (wave == 0) {
        int act = 0, child = 0;
        if (fresh_root) {
            const Position cur = uniform(hist[ply]);
            gen_legal_wave(cur, s_moves, lane, nl);
            wave_sync();
            act = legal_has_move(s_moves, nl, mv, lane) ? 2 : 0;
        } else if (h0.fc >= 1) {
            bool hit = false;
            int at = 0;
            for (int k = lane; k < (int)h0.nc; k += 64)
                if (MV[h0.fc + k] == mv) {
                    hit = true;
                    at = k;
                }
            const unsigned long long mask = __ballot(hit);
            if (mask) {
                act = 1;
                child = h0.fc + __builtin_amdgcn_readlane(at, __ffsll((long long)mask) - 1);
            }
        }   // (a terminal root has no children: no move is playable there)
        if (lane == 0) {
            s_act = act;
            s_child = child;
            s_nexp = 0;
            s_flag[0] = s_flag[1] = s_flag[2] = 0;
        }
    }
    for (int w = tid; w < PS_WORDS; w += ADV_THREADS) s_ps[w] = 0;
    __syncthreads();
    const int act = s_act, cnode = s_child;
    if (act == 0) {
        refuse(-1);
        return;
    }

    // ------------------------------------------------------------ phase B: marks and new indices of [cnode, n); nothing of the slot is written
    uint32_t n_keep = 0, n_keep_exp = 0;
    if (act == 1) {
        if (tid == 0) mark_store(&M[cnode], 1u);
        __syncthreads();
        int bad = 0;
        for (int b = cnode; b < n; b += ADV_THREADS) {
            const int i = b + tid;
            NodeHdr h{-1, 0, 0};
            if (i < n) h = H[i];
            bool expd = i < n && h.fc >= 0;
            if (expd && (h.fc <= i || h.nc < 1 || h.nc > MAXC || (long long)h.fc + h.nc > (long long)n || h.ps < 1 || (int)h.ps >= n_exp_old)) {
                bad = 1;
                expd = false;
            }
            bool done = false;
            for (;;) {
                int changed = 0;
                if (expd && !done && mark_load(&M[i]) != 0u) {
                    for (int k = 0; k < (int)h.nc; k++) mark_store(&M[h.fc + k], 1u);
                    done = true;
                    changed = h.fc < b + ADV_THREADS;
                }
                if (!block_any(changed != 0, s_flag, any_k)) break;
            }
            const bool keep = i < n && mark_load(&M[i]) != 0u;
            uint32_t tot;
            const uint32_t pre = block_excl_scan(keep ? 1u : 0u, s_wsum, &tot);
            if (keep) {
                mark_store(&M[i], n_keep + pre + 1u);
                if (expd) {
                    atomicOr(&s_ps[h.ps >> 5], 1u << (h.ps & 31));
                    atomicAdd(&s_nexp, 1u);
                }
            }
            n_keep += tot;
        }
        __syncthreads();
        // the set bits below every word of the bitmap
        uint32_t cnt = 0;
#pragma unroll
        for (int k = 0; k < PS_WORDS / ADV_THREADS; k++) cnt += (uint32_t)__popc(s_ps[tid * (PS_WORDS / ADV_THREADS) + k]);
        uint32_t below = block_excl_scan(cnt, s_wsum, &n_keep_exp);
#pragma unroll
        for (int k = 0; k < PS_WORDS / ADV_THREADS; k++) {
            s_pre[tid * (PS_WORDS / ADV_THREADS) + k] = below;
            below += (uint32_t)__popc(s_ps[tid * (PS_WORDS / ADV_THREADS) + k]);
        }
        if (n_keep_exp != s_nexp || n_keep < 1u) bad = 1;   // (two kept nodes with one tpos slot)
        if (block_any(bad != 0, s_flag, any_k)) {   // not a tree of this search: nothing has been written
            refuse(-2);
            return;
        }
    }
    auto new_ps = [&](uint32_t ps) { return 1u + s_pre[ps >> 5] + (uint32_t)__popc(s_ps[ps >> 5] & ((1u << (ps & 31)) - 1u)); };

    // ------------------------------------------------------------ phase C (wave 0): trace step, game line, the end of the ply
    if (wave == 0) {
        const Position cur = uniform(hist[ply]);
        const size_t tstep = (size_t)ts * p.num_steps + (size_t)i_step;
        if (act == 1) {   // what the end of a searched ply records
            const int nc = h0.nc, fc = h0.fc;
            for (int k = lane; k < nc; k += 64) {
                p.t_cmove[tstep * MAXC + k] = MV[fc + k];
                p.t_cn[tstep * MAXC + k] = N[fc + k];
                p.t_cq[tstep * MAXC + k] = W[fc + k];
                p.t_cu[tstep * MAXC + k] = U[fc + k];
            }
            if (lane == 0) {
                p.t_move[tstep] = mv;
                p.t_q[tstep] = W[0];
                p.t_nchild[tstep] = nc;
            }
        } else {   // what k_push_moves records: a ply that was not searched
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
        int go_on = 1;
        if (i_step > p.outcome_gate) {
            HistChain hc{hist};
            int winner = -1;
            int term = outcome_claim_draw(hc, new_ply, &winner);
            if (term != T_NONE) {
                wave_sync();
                finish_game(p, g, lane, 1, term, winner);
                go_on = 0;
            }
        }
        if (go_on && (i_step + 1 >= p.num_steps || new_ply + 1 >= p.hist_cap)) {
            wave_sync();
            finish_game(p, g, lane, 0, 0, -1);
            go_on = 0;
        }
        if (lane == 0) {
            if (go_on) tpos[0] = np;
            s_act = go_on ? act : 0;
        }
    }
    __syncthreads();
    if (s_act == 0) {   // the move ended the game
        if (tid == 0) {
            a.status[e] = 1;
            if (a.kept) a.kept[e * 3] = a.kept[e * 3 + 1] = a.kept[e * 3 + 2] = 0;
        }
        return;
    }

    // ------------------------------------------------------------ phase D: the move in place
    if (act == 2) {   // the one-node root k_push_moves leaves
        if (tid == 0) {
            N[0] = 0;
            W[0] = 0.0f;
            P[0] = 0.0f;
            U[0] = 0.0f;
            MV[0] = mv;
            H[0] = NodeHdr{-1, 0, 0};
            c.n_nodes = 1;
            c.n_exp = 1;
            c.sim = 0;
            c.leaf = 0;
            c.path_len = 0;
            a.status[e] = 0;
            if (a.kept) {
                a.kept[e * 3] = 1;
                a.kept[e * 3 + 1] = 1;
                a.kept[e * 3 + 2] = 0;
            }
        }
        return;
    }
    int root_n = 0;   // (thread 0 owns node cnode)
    for (int b = cnode; b < n; b += ADV_THREADS) {   // new index <= old index: a chunk is read whole, then written
        const int i = b + tid;
        const uint32_t m = i < n ? mark_load(&M[i]) : 0u;
        int vn = 0;
        float vw = 0.f, vp = 0.f, vu = 0.f;
        uint16_t vm = 0;
        NodeHdr h{-1, 0, 0};
        if (m) {
            vn = N[i];
            vw = W[i];
            vp = P[i];
            vu = U[i];
            vm = MV[i];
            h = H[i];
            if (h.fc >= 0) {   // (checked in phase B: the block lies in [i + 1, n) and is marked, ps is a set bit)
                h.fc = (int32_t)mark_load(&M[h.fc]) - 1;
                h.ps = (uint16_t)new_ps(h.ps);
            }
            if (i == cnode) {   // the root, as a fresh root has it
                vp = 0.0f;
                vu = 0.0f;
                vm = mv;
                root_n = vn;
            }
        }
        __syncthreads();
        if (m) {
            const uint32_t j = m - 1u;
            N[j] = vn;
            W[j] = vw;
            P[j] = vp;
            U[j] = vu;
            MV[j] = vm;
            H[j] = h;
        }
    }
    __syncthreads();
    const int ps_end = n_exp_old < 65536 ? n_exp_old : 65536;
    for (int b = 0; b < ps_end; b += ADV_THREADS) {   // the kept records in old-ps order from slot 1 (slot 0 holds the root's: phase C)
        const int ps = b + tid;
        const bool has = ps < ps_end && ((s_ps[ps >> 5] >> (ps & 31)) & 1u);
        Position rec{};
        if (has) rec = tpos[ps];
        __syncthreads();
        if (has) tpos[new_ps((uint32_t)ps)] = rec;
    }
    if (tid == 0) {
        c.n_nodes = (int32_t)n_keep;
        c.n_exp = 1 + (int32_t)n_keep_exp;
        c.sim = 0;
        c.leaf = 0;
        c.path_len = 0;
        a.status[e] = 0;
        if (a.kept) {
            a.kept[e * 3] = (int32_t)n_keep;
            a.kept[e * 3 + 1] = 1 + (int32_t)n_keep_exp;
            a.kept[e * 3 + 2] = root_n;
        }
    }
}

}  // namespace sc

namespace scl {
void advance(const sc::SpParams& p, const scad::AdvanceArgs& a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(sc::k_advance, dim3(a.n), dim3(scad::ADV_THREADS), 0, s, p, a);
}
}  // namespace scl
