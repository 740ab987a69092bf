// search_select.hpp -- PUCT search on the GPU, one 64-lane wavefront per concurrent game: the select side (expansion and the game's
// lifecycle: search_expand.hpp).
//
// Rewrites src/mcts.rs (Node/Cursor/uct/find_max/backward/select/mcts/step), the Game::predict front half (legal moves, terminal test,
// _encode: src/backends/torch.rs:89-113, src/chess.rs:845-877) and the per-ply driver of src/main.rs:168-233 as HIP kernels.
//
// Data layout in HBM (per game slot g; all arrays are contiguous per slot so one wave's accesses coalesce): SoA node pool
// N/W/P/U/MV/NC/FC/PS[g*node_cap + i] with the children of a node stored contiguously in python-chess move order (lane = child in PUCT),
// Position records for the game line (hist) and for expanded nodes (tpos), the last path, and the NN input/outputs of the leaf. Priors
// are cached at expansion (the reference re-evaluates the net at every node of every descent, src/mcts.rs:152; the net is deterministic
// so the search is identical).
//
// Scalar chess logic (make_move, move generation) is executed wave-uniformly (all lanes compute the same values: no divergence, no
// broadcasts); PUCT argmax, repetition scan, plane encoding, child initialisation and backup are lane-parallel with wave
// shuffles/ballots.
//
// Bit-exactness, said once for every file of the search: the PUCT arithmetic must round exactly like the reference's f32 expression
// (src/mcts.rs:69-75), which Rust never contracts into FMAs, and the value the search backs up must be the bits `predict` returns.
// mcts_kernels.hip, encode_kernels.hip and score_kernels.hip are built with -ffp-contract=off; nn_kernels.hip and step_kernels.hip (the
// fused k_step: search wave + tower) with contraction on, which the tower's epilogues are written for.  So the search functions of this
// header and of search_expand.hpp carry `#pragma clang fp contract(off)` in their bodies and use raw hardware transcendentals (the
// library's log / exp wrappers expand differently under the two settings): they compile to the same instructions in both units.
// value_tail.hpp, called by dev_expand and by k_value_finish (nn_kernels.hip), does the same and must compile identically in both units
// as well. No kernels here: k_mcts and the test aids are in mcts_kernels.hip, k_step in step_kernels.hip.
#pragma once
#include <type_traits>
#include <hip/hip_runtime.h>

#include "mcts_types.hpp"
#include "position_chain.hpp"

namespace sc {

using scw::dpp_i, scw::wave_sum_fixed, scw::wave_sum_i;

// index of the maximal u over the lanes with idx >= 0; ties go to the LARGER index (Iterator::max_by keeps the last
// maximum, src/mcts.rs:78-88).  u must be finite.  Returns -1 when no lane has a candidate.  Wave-uniform result.
__device__ __forceinline__ int wave_argmax_last(float u, int idx) {
    // order-preserving map of a finite float to unsigned (+0.0 added first: -0.0 and +0.0 compare equal as floats)
    unsigned b = __builtin_bit_cast(unsigned, u + 0.0f);
    unsigned key = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    int hi = idx >= 0 ? (int)key : 0, lo = idx;   // compared as unsigned; lo = -1 marks "none" (never wins: hi = 0 ... see below)
    auto step = [&](int ohi, int olo) {
        const bool take = olo >= 0 && (lo < 0 || (unsigned)ohi > (unsigned)hi || ((unsigned)ohi == (unsigned)hi && olo > lo));
        hi = take ? ohi : hi;
        lo = take ? olo : lo;
    };
    step(dpp_i<0xB1>(hi), dpp_i<0xB1>(lo));
    step(dpp_i<0x4E>(hi), dpp_i<0x4E>(lo));
    step(dpp_i<0x141>(hi), dpp_i<0x141>(lo));
    step(dpp_i<0x140>(hi), dpp_i<0x140>(lo));
    int bh = __builtin_amdgcn_readlane(hi, 0), bl = __builtin_amdgcn_readlane(lo, 0);
#pragma unroll
    for (int r = 16; r < 64; r += 16) {
        const int oh = __builtin_amdgcn_readlane(hi, r), ol = __builtin_amdgcn_readlane(lo, r);
        const bool take = ol >= 0 && (bl < 0 || (unsigned)oh > (unsigned)bh || ((unsigned)oh == (unsigned)bh && ol > bl));
        bh = take ? oh : bh;
        bl = take ? ol : bl;
    }
    return bl;
}
// Same contract for the common case of ONE candidate per lane whose index is its lane number (nodes with <= 64
// children): the wave maximum of the keys (4 DPP max steps), then the HIGHEST lane holding it (ballot + find-last-set)
// -- a third of the instructions of the (key, index) pair reduction above, on every level of every descent.
__device__ __forceinline__ int wave_argmax_last_lane(float u, bool has) {
    unsigned b = __builtin_bit_cast(unsigned, u + 0.0f);
    unsigned key = (b & 0x80000000u) ? ~b : (b | 0x80000000u);   // >= 0x00800000 for every finite float
    int k = has ? (int)key : 0;
    auto umax = [](int a, int b2) { return (int)((unsigned)a > (unsigned)b2 ? (unsigned)a : (unsigned)b2); };
    int m = k;
    m = umax(m, dpp_i<0xB1>(m));
    m = umax(m, dpp_i<0x4E>(m));
    m = umax(m, dpp_i<0x141>(m));
    m = umax(m, dpp_i<0x140>(m));
    const int wm = umax(umax(__builtin_amdgcn_readlane(m, 0), __builtin_amdgcn_readlane(m, 16)),
                        umax(__builtin_amdgcn_readlane(m, 32), __builtin_amdgcn_readlane(m, 48)));
    const unsigned long long mask = __ballot(has && k == wm);
    return mask ? 63 - __clzll((long long)mask) : -1;
}
__device__ __forceinline__ NodeHdr uniform(const NodeHdr& q) {
    NodeHdr r;
    r.fc = uniform(q.fc);
    r.nc = (uint16_t)uniform((int)q.nc);
    r.ps = (uint16_t)uniform((int)q.ps);
    return r;
}
__device__ __forceinline__ GameCtl uniform(const GameCtl& q) {
    GameCtl r;
    r.status = uniform(q.status);
    r.ply = uniform(q.ply);
    r.sim = uniform(q.sim);
    r.n_nodes = uniform(q.n_nodes);
    r.n_exp = uniform(q.n_exp);
    r.leaf = uniform(q.leaf);
    r.path_len = uniform(q.path_len);
    r.leaf_kind = uniform(q.leaf_kind);
    r.n_legal = uniform(q.n_legal);
    r.leaf_value = __builtin_bit_cast(float, uniform(__builtin_bit_cast(int, q.leaf_value)));
    r.err = (uint32_t)uniform((int)q.err);
    r.trace_slot = uniform(q.trace_slot);
    r.game_id = uniform((bb_t)q.game_id);
    r.start_ply = uniform(q.start_ply);
    r.rollout_cur = uniform(q.rollout_cur);
    return r;
}

// ------------------------------------------------------------------ Dirichlet(0.3) root noise
// get_noise (src/mcts.rs:123-130).  The reference draws from thread_rng; here a counter-based
// stream keyed by (seed, game, ply, sim, child) -- parity is distributional only.
__device__ inline float u01_open(uint64_t& st) {
#pragma clang fp contract(off)   // exact f32 like the reference, in either translation unit (top of this file)
    st = mix64(st);
    return ((float)(st >> 40) + 0.5f) * (1.0f / 16777216.0f);
}
// Gamma(0.3, 1) sample for the Dirichlet(0.3) root noise (src/mcts.rs:123-130): Gamma(1.3) by Marsaglia-Tsang times
// U^(1/0.3).  The draw happens for every child at EVERY simulation, on the critical path of the descent, so it uses
// the hardware transcendentals (v_log / v_exp / v_cos / v_sqrt, ~1 ulp) instead of the correctly rounded library
// routines (10x the instructions): the reference's noise comes from thread_rng, parity is distributional
// (tests: test_root_noise_is_dirichlet for the marginal's moments; tests/test_gpu_noise.py holds every sample of both
// builds to the float64 replay of tests/noise_ref.py, whose law tests/test_noise_ref.py checks -- measured there, the
// four functions together stay inside the error bound of correctly rounded ones, 0.5 ulp each).
__device__ inline float gamma03(uint64_t st) {
#pragma clang fp contract(off)   // exact f32 like the reference, in either translation unit (top of this file)
    // raw hardware transcendentals only (v_log_f32 = log2, v_exp_f32 = 2^x): both units must draw the same noise (top of this file)
    const float LN2 = 0.69314718f;
    const float alpha = 0.3f;
    const float boost = __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(u01_open(st)) * (1.0f / alpha));   // u^(1/alpha)
    const float d = alpha + 1.0f - 1.0f / 3.0f;
    const float c = 0.3390317518f;  // 1 / sqrt(9 d)
    for (int it = 0; it < 64; it++) {
        float a = u01_open(st), b = u01_open(st);
        float x = __builtin_amdgcn_sqrtf(-2.0f * LN2 * __builtin_amdgcn_logf(a)) * __builtin_amdgcn_cosf(b);   // v_cos_f32 takes revolutions
        float v = 1.0f + c * x;
        if (v <= 0.0f) continue;
        v = v * v * v;
        float u = u01_open(st);
        if (LN2 * __builtin_amdgcn_logf(u) < 0.5f * x * x + d - d * v + d * (LN2 * __builtin_amdgcn_logf(v))) return boost * d * v;
    }
    return boost * d;
}

// ------------------------------------------------------------------ select (src/mcts.rs:132-227)
constexpr int DEPTH_LDS = 1024;  // path entries tracked in LDS (a deeper path sets ERR_DEPTH_OVERFLOW)

// Cycle stamps of the search's phases (tools/dbg_cycles.py).  Compiled into the kernel that runs every step they cost 0.7 % of
// the headline even while switched off (same-box A/B, tools/ab_r02.py): SC_ST is a template argument of the functions that carry
// them -- true in k_mcts and in the stamped instantiation of the fused step kernel, which the engine launches only while stamps are
// switched on.
#define SC_STAMP(k)                                                                       \
    do {                                                                                  \
        if constexpr (SC_ST) {                                                            \
            if (p.dbg_cycles && lane == 0) p.dbg_cycles[(size_t)g * 32 + (k)] = clock64(); \
        }                                                                                 \
    } while (0)

// Hand-off to a helper wavefront (fused step kernel): once the leaf position and its repetition flags stand, the plane
// encoding (history loads + 7 KB of LDS writes) is independent of move generation; wave 1 of the workgroup, idle during
// the search, does it while this wave generates the moves.  An LDS mailbox: the searching wave writes idx / root_ply,
// then state (1 = encode, 2 = nothing to do, 3 = the leaf's repetition flags first -- answered with state 4 and the flags in
// `pad` --, then encode); the helper polls state.
struct HelperBox {
    int state, idx, root_ply, pad;
};
__device__ __forceinline__ void helper_post(HelperBox* box, int lane, int state, int idx, int root_ply) {
    if (!box) return;
    if (lane == 0) {
        box->idx = idx;
        box->root_ply = root_ply;
    }
    wave_sync();   // the payload (and s_leaf / s_ps before it) has landed in LDS before the state word is written
    if (lane == 0) *reinterpret_cast<volatile int*>(&box->state) = state;
}
// the helper wave: waits for the mailbox, encodes the planes of the leaf into `stage` (and its meta row)
__device__ __forceinline__ void dev_encode_helper(const SpParams& p, int g, int lane, HelperBox* box, int8_t* s_stage, Position* s_leaf_p,
                                                  uint16_t* s_ps, Position* s_hist) {
    int st = 0;
    for (int spin = 0; spin < (1 << 22) && st == 0; spin++) {   // bounded: a wave never hangs on a missing post
        st = *reinterpret_cast<volatile int*>(&box->state);
        if (st == 0) __builtin_amdgcn_s_sleep(2);
    }
    st = __builtin_amdgcn_readfirstlane(st);
    if (st == 0 && lane == 0) atomicOr(&p.cnt->err, ERR_HELPER_TIMEOUT);   // never seen: the search wave posts on every path
    if (st != 1 && st != 3) return;
    wave_sync();
    const int idx = __builtin_amdgcn_readfirstlane(box->idx), root_ply = __builtin_amdgcn_readfirstlane(box->root_ply);
    DevChain ch{p.hist + (size_t)g * p.hist_cap, root_ply, p.tpos + (size_t)g * p.tpos_cap, s_ps, s_leaf_p, idx};
    if (st == 3) {
        // the leaf's repetition flags (move generation does not need them: the search wave is already generating the moves
        // and collects the flags from the mailbox afterwards)
        const bb_t key0 = s_leaf_p->key;
        const uint8_t rf = (uint8_t)__builtin_amdgcn_readfirstlane((int)rep_flags_wave(ch, idx, key0, lane));
        const uint8_t fl = (uint8_t)((s_leaf_p->flags & F_IRREV) | rf);
        wave_sync();   // every lane has read the old flags
        if (lane == 0) {
            s_leaf_p->flags = fl;
            box->pad = fl;
        }
        wave_sync();
        if (lane == 0) *reinterpret_cast<volatile int*>(&box->state) = 4;
    }
    stage_history(ch, idx, lane, s_hist);
    wave_sync();
    encode_wave(s_hist, idx < 7 ? idx + 1 : 8, lane, s_stage, nullptr, p.meta + (size_t)g * 8);
}

// Returns true when the selected leaf needs a network evaluation (planes, legal moves and action indices are then in
// place).  PLANES_TO_HBM = false: the planes stay in s_stage (fused step kernel).  box != nullptr: the planes are encoded
// by the helper wave (above) instead of this one.
template <bool PLANES_TO_HBM = true, bool SC_ST = true>
__device__ __forceinline__ bool dev_select(const SpParams& p, int g, int lane, int8_t* s_stage, move_t* s_moves, Position* s_leaf_p,
                                        uint16_t* s_ps, Position* s_hist, const GameCtl& cs_pre, bool cs_pre_valid,
                                        HelperBox* box = nullptr) {
#pragma clang fp contract(off)
    Position& s_leaf = *s_leaf_p;
    SC_STAMP(2);
    GameCtl& c = p.ctl[g];
    GameCtl cs = cs_pre;
    if (!cs_pre_valid) cs = uniform(c);  // one 64-byte fetch instead of a chain of dependent field loads
    // The root position, the root header and the root's children ride in ONE round trip (their addresses depend on g
    // only: the tree is rebuilt every ply with the root at node 0 and its children at nodes 1..nc, first expansion).
    // As in dev_expand: all loads first, unguarded (clamped index; lanes past the child count are masked where the
    // values are used), and the wave-uniform ones move to SGPRs only after the last load has been issued.
    const Position root_raw = p.tpos[(size_t)g * p.tpos_cap];
    const NodeHdr hdr_raw = p.H[(size_t)g * p.node_cap];
    const size_t nb0 = (size_t)g * p.node_cap + (1 + lane < p.node_cap ? 1 + lane : p.node_cap - 1);
    const int pf_n = p.N[nb0];
    const float pf_w = p.W[nb0], pf_p = p.P[nb0];
    const NodeHdr pf_h = p.H[nb0];
    __builtin_amdgcn_sched_barrier(0);
    const Position root = uniform(root_raw);
    NodeHdr hdr = uniform(hdr_raw);
    if (cs.status != ST_ACTIVE) {
        if (lane == 0) c.leaf_kind = LK_NONE;
        helper_post(box, lane, 2, 0, 0);
        return false;
    }
    const size_t nb = (size_t)g * p.node_cap;
    const int32_t* N = p.N + nb;
    const float* W = p.W + nb;
    const float* P = p.P + nb;
    float* U = p.U + nb;
    const uint16_t* MV = p.MV + nb;
    const NodeHdr* H = p.H + nb;
    int32_t* path = p.path + (size_t)g * p.max_depth;
    const Position* hist = p.hist + (size_t)g * p.hist_cap;
    Position* tpos = p.tpos + (size_t)g * p.tpos_cap;
    const int root_ply = cs.ply;
    const int root_turn = root.turn;
    const int dmax = p.max_depth < DEPTH_LDS ? p.max_depth : DEPTH_LDS;

    int node = 0, depth = 0, parent_ps = 0;
    if (lane == 0) {
        path[0] = 0;
        s_ps[0] = 0;
    }
    uint32_t err = 0;
    for (;;) {
        const int nc = hdr.nc;
        if (nc == 0) break;
        const int fc = hdr.fc;
        // One level of the descent, generic in the number of 64-child rounds it is compiled for: nodes with more than
        // 64 children are rare (the common case is ONE round), and the 4-round code carries four sets of statistics,
        // guards and selects through the PUCT arithmetic of every level.
        const int nr = (nc + 63) >> 6;  // rounds of 64 children (wave-uniform): usually 1
        int best_i = 0;
        NodeHdr nxt;
        auto level = [&](auto nrc) {
#pragma clang fp contract(off)
            constexpr int NRM = decltype(nrc)::value;
            // children statistics AND their headers in one round trip (lane owns children lane, lane+64, ...)
            int cn[NRM];
            float cw[NRM], cp[NRM];
            NodeHdr ch_[NRM];
#pragma unroll
            for (int r = 0; r < NRM; r++) {
                cn[r] = 0;
                cw[r] = 0.f;
                cp[r] = 0.f;
                ch_[r] = NodeHdr{-1, 0, 0};
                if (r < nr) {
                    int i = lane + 64 * r;
                    bool ok = i < nc;
                    if (r == 0 && depth == 0 && fc == 1) {   // prefetched with the control block
                        cn[0] = ok ? pf_n : 0;
                        cw[0] = ok ? pf_w : 0.f;
                        cp[0] = ok ? pf_p : 0.f;
                        ch_[0] = ok ? pf_h : NodeHdr{-1, 0, 0};
                    } else {
                        cn[r] = ok ? N[fc + i] : 0;
                        cw[r] = ok ? W[fc + i] : 0.f;
                        cp[r] = ok ? P[fc + i] : 0.f;
                        ch_[r] = ok ? H[fc + i] : NodeHdr{-1, 0, 0};
                    }
                }
            }
            if (nc > 1) {
                // side to move at `node`: root_turn flipped per depth; reverse_q = Black to move (torch.rs:49-52)
                const bool reverse_q = ((root_turn ^ (depth & 1)) == BLACK);
                const bool noisy = depth == 0 && p.with_noise;
                float* nz = p.noise + (size_t)g * MAXC;
                float nzv[NRM];
#pragma unroll
                for (int r = 0; r < NRM; r++) nzv[r] = 0.f;
                if (noisy) {
                    if (!p.external_noise) {
                        float gsum = 0.0f;
#pragma unroll
                        for (int r = 0; r < NRM; r++) {
                            int i = lane + 64 * r;
                            if (i < nc) {
                                nzv[r] = gamma03(sc_rng(p.seed, cs.game_id, (uint64_t)root_ply, 3, (uint64_t)cs.sim * 256 + (uint64_t)i));
                                gsum += nzv[r];
                            }
                        }
                        gsum = wave_sum_fixed(gsum);
#pragma unroll
                        for (int r = 0; r < NRM; r++) {
                            int i = lane + 64 * r;
                            nzv[r] = nzv[r] / gsum;
                            if (i < nc) nz[i] = nzv[r];
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < NRM; r++) {
                            int i = lane + 64 * r;
                            if (i < nc) nzv[r] = nz[i];
                        }
                    }
                }
                int tot = 0;
#pragma unroll
                for (int r = 0; r < NRM; r++) tot += cn[r];
                tot = wave_sum_i(tot);
                const float sqrt_total = sqrtf((float)tot);
                float best_u = 0.0f;
                best_i = -1;
#pragma unroll
                for (int r = 0; r < NRM; r++) {
                    int i = lane + 64 * r;
                    if (r < nr && i < nc) {
                        float prior = cp[r];
                        if (noisy) prior = prior * (1.0f - p.epsilon) + nzv[r] * p.epsilon;  // mcts.rs:181
                        // uct(): src/mcts.rs:69-75
                        float average_award = cw[r] / ((float)cn[r] + 1e-4f) * (reverse_q ? -1.0f : 1.0f);
                        float exploration = (sqrt_total + 0.01f) / (1.0f + (float)cn[r]) * p.cpuct * prior;
                        float u = average_award + exploration;
                        U[fc + i] = u;
                        if (!isfinite(u)) err |= ERR_NONFINITE_UCT;
                        if (best_i < 0 || u >= best_u) {  // later index wins ties (max_by keeps the last maximum)
                            best_u = u;
                            best_i = i;
                        }
                    }
                }
                if constexpr (NRM == 1) best_i = wave_argmax_last_lane(best_u, best_i >= 0);   // best_i is the lane number here
                else best_i = wave_argmax_last(best_u, best_i);
            }
            best_i = __builtin_amdgcn_readfirstlane(best_i);
            // header of the chosen child: owned by lane best_i & 63, register best_i >> 6
            const int rr = best_i >> 6;
            NodeHdr mine = ch_[0];
#pragma unroll
            for (int r = 1; r < NRM; r++)
                if (rr == r) mine = ch_[r];
            nxt.fc = __builtin_amdgcn_readlane(mine.fc, best_i & 63);
            int packed = __builtin_amdgcn_readlane((int)mine.nc | ((int)mine.ps << 16), best_i & 63);
            nxt.nc = (uint16_t)(packed & 0xffff);
            nxt.ps = (uint16_t)((unsigned)packed >> 16);
        };
        if (nr == 1) level(std::integral_constant<int, 1>{});
        else level(std::integral_constant<int, 4>{});
        parent_ps = hdr.ps;
        node = fc + best_i;
        hdr = nxt;
        depth++;
        if (depth >= dmax) {
            err |= ERR_DEPTH_OVERFLOW;
            depth--;
            break;
        }
        if (lane == 0) {
            path[depth] = node;
            s_ps[depth] = hdr.ps;
        }
    }
    SC_STAMP(3);
    if (p.dbg_cycles && lane == 0) p.dbg_cycles[(size_t)g * 32 + 7] = depth;   // developer stamp: levels walked
    unsigned long long anyerr = __ballot(err != 0);
    if (anyerr) {
        for (int o = 32; o > 0; o >>= 1) err |= __shfl_xor(err, o, 64);
        if (lane == 0) {
            c.err = cs.err | err;
            atomicOr(&p.cnt->err, (int)err);
        }
    }
    const int fcl = hdr.fc;
    if (lane == 0) {
        c.leaf = node;
        c.path_len = depth + 1;
    }
    if (fcl <= -2) {  // terminal seen before: predict() returns the same outcome again (torch.rs:98-106)
        if (lane == 0) {
            c.leaf_kind = LK_TERM_CACHED;
            c.leaf_value = fcl == -2 ? 0.0f : fcl == -3 ? 1.0f : -1.0f;
            c.n_legal = 0;
        }
        helper_post(box, lane, 2, 0, 0);
        return false;
    }
    // position of the leaf (wave-uniform)
    Position pos;
    if (depth == 0) {
        pos = root;
    } else {
        pos = uniform(tpos[parent_ps]);
        make_move(pos, (move_t)__builtin_amdgcn_readfirstlane((int)MV[node]));  // state.advance (mcts.rs:224)
    }
    if (lane == 0) s_leaf = pos;
    wave_sync();  // s_leaf, s_ps visible
    DevChain ch{hist, root_ply, tpos, s_ps, &s_leaf, root_ply + depth};
    const bool rep_by_helper = box && depth > 0;   // the helper wave scans for repetitions too (a round trip off this wave's chain)
    if (depth > 0 && !box) {
        uint8_t rf = (uint8_t)__builtin_amdgcn_readfirstlane((int)rep_flags_wave(ch, root_ply + depth, pos.key, lane));
        pos.flags = (uint8_t)((pos.flags & F_IRREV) | rf);
        wave_sync();
        if (lane == 0) s_leaf.flags = pos.flags;
        wave_sync();
    }
    SC_STAMP(4);
    // history for the encoder: issued now so the loads overlap move generation -- or the whole encoding handed to the
    // helper wave (a terminal leaf wastes its work: nothing reads the planes then)
    if (box) helper_post(box, lane, rep_by_helper ? 3 : 1, root_ply + depth, root_ply);
    else stage_history(ch, root_ply + depth, lane, s_hist);
    // scratch slot for the expansion (claimed in dev_expand if the leaf is not terminal); with the helper's flags: below
    if (lane == 0 && !rep_by_helper) tpos[cs.n_exp] = pos;
    int n = 0;
    bool in_check = gen_legal_wave(pos, s_moves, lane, n);   // lane = square (chess_rules_wave.hpp)
    wave_sync();
    SC_STAMP(5);
    // --rollout-factor (src/main.rs:175-176): the ply's budget follows from the root's legal-move count, known here at
    // the first simulation of the ply (the only one whose leaf is the root)
    if (depth == 0 && p.rollout_factor > 0.f && lane == 0) {
        const int r = (int)((float)n * p.rollout_factor);
        c.rollout_cur = r < 300 ? r : 300;
    }
    if (n == 0) {
        if (lane == 0) {
            c.leaf_kind = LK_TERM_NEW;
            // winner -> +1 white / -1 black / 0 (torch.rs:100-104); checkmated side is the one to move
            c.leaf_value = in_check ? (pos.turn == WHITE ? -1.0f : 1.0f) : 0.0f;
            c.n_legal = 0;
        }
        return false;
    }
    uint16_t* lm = p.legal_mv + (size_t)g * MAXC;
    uint16_t* li = p.legal_idx + (size_t)g * MAXC;
    uint32_t bad = 0;
    for (int i = lane; i < n; i += 64) {
        move_t m = s_moves[i];
        int idx = move_index(m, pos.turn);
        if (idx < 0) {
            bad = 1;
            idx = 0;
        }
        lm[i] = m;
        li[i] = (uint16_t)idx;
    }
    if (__ballot(bad) && lane == 0) {
        c.err = cs.err | err | ERR_BAD_MOVE_INDEX;
        atomicOr(&p.cnt->err, ERR_BAD_MOVE_INDEX);
    }
    if (rep_by_helper) {
        int st = 3;
        for (int spin = 0; spin < (1 << 22) && st != 4; spin++) {   // (long answered: the scan is shorter than move generation)
            st = *reinterpret_cast<volatile int*>(&box->state);
            if (st != 4) __builtin_amdgcn_s_sleep(1);
        }
        st = __builtin_amdgcn_readfirstlane(st);
        wave_sync();
        if (st != 4 && lane == 0) atomicOr(&p.cnt->err, ERR_HELPER_TIMEOUT);
        pos.flags = (uint8_t)__builtin_amdgcn_readfirstlane(box->pad);
        if (lane == 0) tpos[cs.n_exp] = pos;
    }
    const int idx = root_ply + depth;
    if (!box) encode_wave(s_hist, idx < 7 ? idx + 1 : 8, lane, s_stage, PLANES_TO_HBM ? p.boards + (size_t)g * 7168 : nullptr, p.meta + (size_t)g * 8);
    if (lane == 0) {
        c.leaf_kind = LK_EVAL;
        c.n_legal = n;
        p.n_legal[g] = n;
    }
    SC_STAMP(6);
    return true;
}

}  // namespace sc
