// perft_kernels.hip -- perft on the device (sc_perft): node counts, the divide and the kinds of the last moves, any position.
//
// A breadth-first frontier of 72-byte node records in HBM, one level buffer per depth, walked by the host (perft.hip), which cuts
// a level where its children outgrow the next buffer.  Every kernel handles a node with one wavefront and generates its legal
// moves with gen_legal_wave into the wave's own 448 bytes of LDS; a workgroup is four such waves that share nothing, so no kernel
// holds a workgroup barrier between them (wave_sync orders a wave's LDS stores and loads) and none waits for another workgroup.
//
//   k_perft_roots      one wavefront per entry: its base or the start position, its moves replayed with every move looked up
//       among the generated legal moves (legal_has_move), the root record or the failing ply; the legal moves of the
//       root are the divide row's moves.
//   k_perft_count      legal moves per node -> uint32.  On the last level that is the node's share of the total ("bulk counting":
//       no record is made for depth `depth`).
//   (scan)             the host scans the counts with scl::exclusive_scan_u32 (scan_kernels.hip): a node's first child slot, the
//       total behind the last.  Children lie in frontier order and, within a node, in generator order: the oracle's enumeration order.
//   k_perft_expand     generates again -- 6 k cycles of a wave that would otherwise wait for a 448-byte row to come back from
//       HBM, and 448 B a node is six times the record -- then lane l makes children l, l + 64, l + 128, l + 192 with the scalar
//       make_move<false> on its own registers and stores them at the node's offset.  The count is compared with the scan's.
//   k_perft_leaf_kinds the last level with kinds: each lane classifies its moves against the parent (target occupied or en
//       passant, the king moving two files, promotion bits), makes the child and looks for attackers of the child's king;
//       only for children in check the wave walks the ballot, broadcasts the child and generates: an empty list is a mate.
//   k_perft_attribute  the last level's counts summed by root move.  The frontier is ordered by root move, so a thread sums a run
//       of 16 consecutive nodes and a workgroup 4 096; what is left at the end of each thread's run is combined through LDS and
//       leaves the workgroup as ONE 64-bit atomic per counter and root move that the workgroup saw.  Integer sums: any order
//       gives the same bits.
//
// Every store goes through an index that was compared with its buffer's capacity; a mismatch sets a bit of the error word.
#include "position_chain.hpp"

#include "launchers.hpp"

namespace scpf {

using namespace sc;
typedef unsigned long long u64;

// the node of a wave (the same address in every lane) as a wave-uniform position
__device__ __forceinline__ Position node_position(const Node& nd) {
    Position p;
#pragma unroll
    for (int t = 0; t < 6; t++) p.pcs[t] = uniform((bb_t)nd.pcs[t]);
    p.occ[0] = uniform((bb_t)nd.occ[0]);
    p.occ[1] = uniform((bb_t)nd.occ[1]);
    p.key = 0;
    p.turn = (uint8_t)uniform((int)nd.turn);
    p.castling = (uint8_t)uniform((int)nd.castling);
    p.ep = (int8_t)uniform((int)nd.ep);
    p.flags = 0;
    p.halfmove = 0;
    p.fullmove = 1;
    return p;
}
__device__ __forceinline__ void store_node(Node* dst, const Position& p, uint32_t root) {
#pragma unroll
    for (int t = 0; t < 6; t++) dst->pcs[t] = p.pcs[t];
    dst->occ[0] = p.occ[0];
    dst->occ[1] = p.occ[1];
    dst->turn = p.turn;
    dst->castling = p.castling;
    dst->ep = p.ep;
    dst->pad = 0;
    dst->root = root;
}
// the board lane `sel` holds (sel wave-uniform), in every lane
__device__ __forceinline__ Position from_lane(const Position& q, int sel) {
    Position r;
#pragma unroll
    for (int t = 0; t < 6; t++) r.pcs[t] = scw::from_lane(q.pcs[t], sel);
    r.occ[0] = scw::from_lane(q.occ[0], sel);
    r.occ[1] = scw::from_lane(q.occ[1], sel);
    r.key = 0;
    r.turn = (uint8_t)__builtin_amdgcn_readlane((int)q.turn, sel);
    r.castling = (uint8_t)__builtin_amdgcn_readlane((int)q.castling, sel);
    r.ep = (int8_t)__builtin_amdgcn_readlane((int)q.ep, sel);
    r.flags = 0;
    r.halfmove = 0;
    r.fullmove = 1;
    return r;
}
__device__ __forceinline__ void raise(uint32_t* err, uint32_t bit) { atomicOr(err, bit); }

// ------------------------------------------------------------------ roots
__global__ __launch_bounds__(64) void k_perft_roots(RootArgs a) {
    const int j = blockIdx.x, lane = threadIdx.x;
    if (j >= a.n) return;
    const int e = a.e0 + j;
    __shared__ move_t s_moves[ROW];
    Position cur = chain_start(a.bases, e, false);
    const uint32_t m0 = a.move_off ? (uint32_t)uniform((int)a.move_off[e]) : 0u;
    const uint32_t m1 = a.move_off ? (uint32_t)uniform((int)a.move_off[e + 1]) : 0u;   // the host checked m1 - m0 <= 4000
    int st = 0;
    for (uint32_t q = m0; q < m1; q++) {
        const move_t mv = (move_t)uniform((int)a.moves[q]);
        int nl = 0;
        gen_legal_wave(cur, s_moves, lane, nl);
        wave_sync();
        const bool found = legal_has_move(s_moves, nl, mv, lane);
        wave_sync();   // the list is read before the next generation writes it
        if (!found) {
            st = -(int)(q - m0 + 1);
            break;
        }
        make_move<false>(cur, mv);
    }
    int nd = 0;
    if (st == 0 && (a.n_div || a.div_moves)) {
        gen_legal_wave(cur, s_moves, lane, nd);
        wave_sync();
    }
    if (a.div_moves)
        for (int k = lane; k < ROW; k += 64) a.div_moves[(size_t)e * ROW + k] = k < nd ? s_moves[k] : (move_t)0;
    if (lane == 0) {
        a.status[e] = st;
        if (a.n_div) a.n_div[e] = nd;
        if (a.out) {
            if ((uint32_t)j < a.cap) store_node(a.out + j, cur, st == 0 ? ((uint32_t)e << 8) | NO_MOVE : DEAD);
            else raise(a.err, ERR_SLOT);
        }
    }
}

// depth 1: every legal move of an entry is one leaf
__global__ __launch_bounds__(256) void k_perft_div_ones(int n, const int32_t* n_div, u64* div_nodes) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * ROW) return;
    if ((int)(i % ROW) < n_div[i / ROW]) div_nodes[i] = 1;
}

// ------------------------------------------------------------------ count
__global__ __launch_bounds__(256) void k_perft_count(Level lv, uint32_t* cnt) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t i = (uint32_t)uniform((int)(blockIdx.x * 4u + (uint32_t)wv));
    if (i >= lv.n) return;
    __shared__ move_t s_moves[4][ROW];
    const Node& nd = lv.nodes[lv.first + i];
    int nl = 0;
    if ((uint32_t)uniform((int)nd.root) != DEAD) {
        const Position p = node_position(nd);
        gen_legal_wave(p, s_moves[wv], lane, nl);
    }
    if (lane == 0) cnt[lv.first + i] = (uint32_t)nl;
}

// ------------------------------------------------------------------ expand
__global__ __launch_bounds__(256) void k_perft_expand(ExpandArgs a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t i = (uint32_t)uniform((int)(blockIdx.x * 4u + (uint32_t)wv));
    if (i >= a.lv.n) return;
    __shared__ move_t s_moves[4][ROW];
    const Node& nd = a.lv.nodes[a.lv.first + i];
    const uint32_t root = (uint32_t)uniform((int)nd.root);
    const uint32_t at = (uint32_t)uniform((int)a.off[a.lv.first + i]), next = (uint32_t)uniform((int)a.off[a.lv.first + i + 1]);
    if (root == DEAD) {
        if (next != at && lane == 0) raise(a.err, ERR_COUNT);
        return;
    }
    const Position p = node_position(nd);
    int nl = 0;
    gen_legal_wave(p, s_moves[wv], lane, nl);
    wave_sync();
    if ((uint32_t)nl != next - at || at < a.base) {   // the scan's count is what the slots were laid out for
        if (lane == 0) raise(a.err, ERR_COUNT);
        return;
    }
    for (int k = lane; k < nl; k += 64) {
        Position c = p;
        make_move<false>(c, s_moves[wv][k]);
        const uint32_t slot = at - a.base + (uint32_t)k;
        if (slot < a.cap) store_node(a.out + slot, c, a.from_roots ? (root & ~255u) | (uint32_t)k : root);
        else raise(a.err, ERR_SLOT);
    }
}

// ------------------------------------------------------------------ the last level with kinds
__global__ __launch_bounds__(256) void k_perft_leaf_kinds(Level lv, LeafOut lo) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t i = (uint32_t)uniform((int)(blockIdx.x * 4u + (uint32_t)wv));
    if (i >= lv.n) return;
    __shared__ move_t s_moves[4][ROW];
    __shared__ move_t s_reply[4][ROW];   // the list of a child in check: only its length is read
    const Node& nd = lv.nodes[lv.first + i];
    int nl = 0;
    unsigned packed = 0;   // this lane's captures | ep << 8 | castles << 16 | promotions << 24: no field of the wave's sum passes 218
    int checks = 0, mates = 0;
    if ((uint32_t)uniform((int)nd.root) != DEAD) {
        const Position p = node_position(nd);
        gen_legal_wave(p, s_moves[wv], lane, nl);
        wave_sync();
        const int us = p.turn;
        const bb_t theirs = occ_c(p, !us);
        for (int k0 = 0; k0 < nl; k0 += 64) {   // nl <= 224: at most four passes
            const int k = k0 + lane;
            Position c = p;
            bool chk = false;
            if (k < nl) {
                const move_t m = s_moves[wv][k];
                const int from = mv_from(m), to = mv_to(m);
                const bool pawn = (p.pcs[PAWN] >> from) & 1, king = (p.pcs[KING] >> from) & 1;
                const bool ep = pawn && to == p.ep && ((from ^ to) & 7) != 0 && !((theirs >> to) & 1);
                const bool cap = ep || ((theirs >> to) & 1);
                const bool castle = king && (to - from == 2 || from - to == 2);
                packed += (cap ? 1u : 0u) | (ep ? 1u << 8 : 0u) | (castle ? 1u << 16 : 0u) | (mv_promo(m) ? 1u << 24 : 0u);
                make_move<false>(c, m);
                const bb_t kbb = c.pcs[KING] & occ_c(c, c.turn);
                if (kbb) chk = attackers_mask(c, us, msb(kbb), all_occ(c)) != 0;
            }
            unsigned long long in_check = __ballot(chk);
            checks += __popcll(in_check);
            while (in_check) {   // at most 64 turns
                const int sel = uniform(__ffsll((long long)in_check) - 1);
                in_check &= in_check - 1;
                const Position child = from_lane(c, sel);
                int nr = 0;
                gen_legal_wave(child, s_reply[wv], lane, nr);
                wave_sync();
                mates += nr == 0 ? 1 : 0;
            }
        }
    }
    const unsigned sum = (unsigned)scw::wave_sum_i((int)packed);
    if (lane == 0) {
        lo.cnt[lv.first + i] = (uint32_t)nl;
        lo.kinds[2 * (size_t)(lv.first + i)] = sum;
        lo.kinds[2 * (size_t)(lv.first + i) + 1] = (uint32_t)checks | ((uint32_t)mates << 8);
    }
}

// ------------------------------------------------------------------ the last level's counts summed by root move
constexpr int SLOTS = 7;   // nodes and the six kinds
__device__ __forceinline__ void add_total(const Totals& t, uint32_t key, int slot, u64 v) {
    if (key == DEAD || v == 0) return;
    const uint32_t e = key >> 8, mv = key & 255u;
    if (e >= (uint32_t)t.n_entries || (mv != NO_MOVE && mv >= (uint32_t)ROW)) {
        raise(t.err, ERR_ENTRY);
        return;
    }
    if (slot == 0) {
        atomicAdd(t.nodes + e, v);
        if (t.div_nodes && mv != NO_MOVE) atomicAdd(t.div_nodes + (size_t)e * ROW + mv, v);
    } else if (t.kinds) {
        atomicAdd(t.kinds + (size_t)e * KINDS + slot, v);
    }
}
__global__ __launch_bounds__(256) void k_perft_attribute(Level lv, LeafOut lo, Totals t) {
    __shared__ uint32_t s_key[256];
    __shared__ u64 s_val[SLOTS][256];
    const int tid = threadIdx.x;
    const bool with_kinds = lo.kinds != nullptr;
    const uint32_t i0 = (blockIdx.x * 256u + (uint32_t)tid) * (uint32_t)ATTR_RUN;   // lv.n <= 2^24
    uint32_t key = DEAD;
    u64 s[SLOTS];
#pragma unroll
    for (int j = 0; j < SLOTS; j++) s[j] = 0;
    for (int r = 0; r < ATTR_RUN; r++) {
        const uint32_t i = i0 + (uint32_t)r;
        if (i >= lv.n) break;
        const uint32_t k = lv.nodes[lv.first + i].root;
        if (k == DEAD) continue;
        if (k != key) {   // a root move ends inside this thread's run: its sums are complete here or continue in no later thread
#pragma unroll
            for (int j = 0; j < SLOTS; j++) {
                add_total(t, key, j, s[j]);
                s[j] = 0;
            }
            key = k;
        }
        s[0] += lo.cnt[lv.first + i];   // 64-bit from the first addition
        if (with_kinds) {
            const uint32_t a = lo.kinds[2 * (size_t)(lv.first + i)], b = lo.kinds[2 * (size_t)(lv.first + i) + 1];
            s[1] += a & 255u;
            s[2] += (a >> 8) & 255u;
            s[3] += (a >> 16) & 255u;
            s[4] += a >> 24;
            s[5] += b & 255u;
            s[6] += (b >> 8) & 255u;
        }
    }
    s_key[tid] = key;
#pragma unroll
    for (int j = 0; j < SLOTS; j++) s_val[j][tid] = s[j];
    __syncthreads();
    // thread j walks the 256 remainders of counter j in frontier order: one atomic per root move the workgroup ends with
    if (tid < (with_kinds ? SLOTS : 1)) {
        uint32_t cur = DEAD;
        u64 acc = 0;
        for (int q = 0; q < 256; q++) {
            const uint32_t k = s_key[q];
            if (k == DEAD) continue;
            if (k != cur) {
                add_total(t, cur, tid, acc);
                cur = k;
                acc = 0;
            }
            acc += s_val[tid][q];
        }
        add_total(t, cur, tid, acc);
    }
}

}  // namespace scpf

namespace scl {
using namespace scpf;
void perft_roots(const RootArgs& a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(k_perft_roots, dim3(a.n), dim3(64), 0, s, a);
}
void perft_div_ones(int n, const int32_t* d_n_div, unsigned long long* d_div_nodes, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_perft_div_ones, dim3((unsigned)(((size_t)n * ROW + 255) / 256)), dim3(256), 0, s, n, d_n_div, d_div_nodes);
}
void perft_count(const Level& lv, uint32_t* d_cnt, hipStream_t s) {
    if (lv.n == 0) return;
    hipLaunchKernelGGL(k_perft_count, dim3((lv.n + 3) / 4), dim3(256), 0, s, lv, d_cnt);
}
void perft_expand(const ExpandArgs& a, hipStream_t s) {
    if (a.lv.n == 0) return;
    hipLaunchKernelGGL(k_perft_expand, dim3((a.lv.n + 3) / 4), dim3(256), 0, s, a);
}
void perft_leaf(const Level& lv, const LeafOut& lo, const Totals& t, hipStream_t s) {
    if (lv.n == 0) return;
    if (lo.kinds) hipLaunchKernelGGL(k_perft_leaf_kinds, dim3((lv.n + 3) / 4), dim3(256), 0, s, lv, lo);
    else hipLaunchKernelGGL(k_perft_count, dim3((lv.n + 3) / 4), dim3(256), 0, s, lv, lo.cnt);
    const unsigned per = 256u * ATTR_RUN;
    hipLaunchKernelGGL(k_perft_attribute, dim3((lv.n + per - 1) / per), dim3(256), 0, s, lv, lo, t);
}
}  // namespace scl
