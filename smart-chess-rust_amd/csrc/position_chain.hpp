// position_chain.hpp -- the chain of positions a wave looks back over (game line, tree path, leaf), its repetition scan,
// the plane encoder (_encode), and for the kernels that rebuild a line from its moves the replay step, the lookup of a move among
// the legal moves and the checked replay made of the two.  Device functions only.
#pragma once
#include <hip/hip_runtime.h>

#include "chess_history.hpp"
#include "chess_rules_wave.hpp"
#include "encode_types.hpp"
#include "wave_util.hpp"

namespace sc {

using scw::uniform, scw::wave_sync;
__device__ __forceinline__ Position uniform(const Position& q) {
    Position r;
#pragma unroll
    for (int t = 0; t < 6; t++) r.pcs[t] = uniform(q.pcs[t]);
    r.occ[0] = uniform(q.occ[0]);
    r.occ[1] = uniform(q.occ[1]);
    r.key = uniform(q.key);
    r.turn = (uint8_t)uniform((int)q.turn);
    r.castling = (uint8_t)uniform((int)q.castling);
    r.ep = (int8_t)uniform((int)q.ep);
    r.flags = (uint8_t)uniform((int)q.flags);
    r.halfmove = (uint16_t)uniform((int)q.halfmove);
    r.fullmove = (uint16_t)uniform((int)q.fullmove);
    return r;
}

// The position a replay of game g starts from: its base (a validated record: key set, flags clear) where the call has bases and
// the game's index is >= 0, else the start position.  keyed: with its transposition key; else key and flags are 0 (boards alone)
__device__ __forceinline__ Position chain_start(const Bases& b, int g, bool keyed) {
    Position cur;
    const int bi = b.rec ? uniform(b.idx[g]) : -1;
    if (bi >= 0) {
        cur = uniform(b.rec[bi]);
    } else {
        set_startpos(cur);
        if (keyed) cur.key = position_key(cur);
    }
    if (!keyed) cur.key = cur.flags = 0;
    return cur;
}

// chain of positions: game history, then the tree path, then the leaf being created
struct DevChain {
    const Position* hist;
    int root_ply;
    const Position* tpos;
    const uint16_t* ps_by_depth;  // LDS: tpos slot of the path node at depth d (expanded nodes only)
    const Position* leaf;
    int leaf_idx;
    __device__ const Position& pos(int i) const {
        if (i <= root_ply) return hist[i];
        if (i == leaf_idx) return *leaf;
        return tpos[ps_by_depth[i - root_ply]];
    }
};
struct HistChain {
    const Position* hist;
    __device__ const Position& pos(int i) const { return hist[i]; }
};

// is_repetition(2) / is_repetition(3) of the position at chain index idx, lane-parallel.
// Lane L looks at i = idx-L: the walk of python-chess is_repetition stops at the first i whose
// incoming move was irreversible, and compares pos(i-1) otherwise.
template <class Chain>
__device__ inline uint8_t rep_flags_wave(const Chain& ch, int idx, bb_t key0, int lane) {
    int matches = 0;
    for (int base = 0;; base += 64) {
        int i = idx - base - lane;
        bool valid = i >= 1;
        bool irrev = false, match = false;
        if (valid) {
            irrev = (ch.pos(i).flags & F_IRREV) != 0;
            match = ch.pos(i - 1).key == key0;
        }
        unsigned long long stopmask = __ballot(irrev || !valid);
        unsigned long long matchmask = __ballot(match && valid);
        bool stopped = stopmask != 0;
        if (stopped) {
            int first = __ffsll((long long)stopmask) - 1;
            matchmask &= first == 0 ? 0ULL : (~0ULL >> (64 - first));
        }
        matches += __popcll(matchmask);
        if (stopped || matches >= 2) break;
    }
    return (uint8_t)((matches >= 1 ? F_REP2 : 0) | (matches >= 2 ? F_REP3 : 0));
}

// Stage the <=8 positions _encode looks at (idx, idx-1, ...) into LDS with two dependent round trips in total:
// lane l fetches 8-byte word (l & 7) [and word 8/9 for l&7 < 2] of history entry l >> 3.
template <class Chain>
__device__ inline void stage_history(const Chain& ch, int idx, int lane, Position* s_hist) {
    const int j = lane >> 3, w = lane & 7;
    if (j <= idx) {
        const unsigned long long* src = reinterpret_cast<const unsigned long long*>(&ch.pos(idx - j));
        unsigned long long* dst = reinterpret_cast<unsigned long long*>(&s_hist[j]);
        dst[w] = src[w];
        if (w < 2) dst[8 + w] = src[8 + w];
    }
}

// _encode (src/chess.rs:845-877) for the position at history depth 0 of s_hist (newest first): lane = output
// pixel.  stage: 7168 B of LDS; out: int8[64][112] in HBM.
__device__ inline void encode_wave(const Position* s_hist, int n_hist, int lane, int8_t* stage, int8_t* out, int32_t* meta_out) {
    uint4* cell16 = reinterpret_cast<uint4*>(stage + lane * 112);
#pragma unroll
    for (int k = 0; k < 7; k++) cell16[k] = make_uint4(0, 0, 0, 0);
    int8_t* cell = stage + lane * 112;
    const int turn = s_hist[0].turn;
    int src = turn == BLACK ? (lane ^ 56) : lane;
    bb_t sb = bit(src);
    for (int j = 0; j < n_hist; j++) {
        const Position& h = s_hist[j];
        bb_t ow = h.occ[WHITE], ob = h.occ[BLACK];
        if ((ow | ob) & sb) {
            int t = 0;
#pragma unroll
            for (int k = 1; k < 6; k++)
                if (h.pcs[k] & sb) t = k;
            int is_white = (ow & sb) ? 1 : 0;
            int mover_side = turn == BLACK ? !is_white : is_white;
            cell[14 * j + t + (mover_side ? 0 : 6)] = 1;
        }
        uint8_t f = h.flags;
        cell[14 * j + 12] = (f & F_REP2) ? 1 : 0;
        cell[14 * j + 13] = (f & F_REP3) ? 1 : 0;
    }
    if (out) {   // (the fused step kernel hands the planes to the network in LDS: no copy to HBM)
        uint4* o16 = reinterpret_cast<uint4*>(out + lane * 112);
#pragma unroll
        for (int k = 0; k < 7; k++) o16[k] = cell16[k];
    }
    if (lane == 0) {
        int32_t m[7];
        encode_meta(s_hist[0], m);
#pragma unroll
        for (int k = 0; k < 7; k++) meta_out[k] = m[k];
        meta_out[7] = 0;
    }
}

// the meta row of ply g as k_steps_dist and k_san_dist write it (lanes 0..6): with apply_mirror that of Board::rotate()
__device__ __forceinline__ void write_meta_row(const RowOut& o, int g, int lane) {
    if (!o.meta || lane >= 7) return;
    const int32_t* m = o.meta_s + (size_t)g * 7;
    int32_t v = m[lane];
    if (o.apply_mirror) v = lane == 0 ? 1 - m[0] : lane == 1 ? m[1] + (m[0] == 1 ? 1 : 0) : lane == 2 ? m[4] : lane == 3 ? m[5] : lane == 4 ? m[2] : lane == 5 ? m[3] : v;
    if (o.layout == 1) static_cast<float*>(o.meta)[(size_t)g * 7 + lane] = (float)v;
    else static_cast<int32_t*>(o.meta)[(size_t)g * 7 + lane] = v;
}

// transposition key of a position, lane = square: the same value as position_key() (XOR of the per-(piece, square) keys and the
// state key), a wave XOR instead of a 32-iteration scalar loop
__device__ inline bb_t position_key_wave(const Position& p, int lane, bool ep_legal) {
    bb_t h = 0;
    if ((all_occ(p) >> lane) & 1) h = psq_key(piece_type_at(p, lane), (int)((p.occ[WHITE] >> lane) & 1), lane);
    unsigned lo = (unsigned)h, hi = (unsigned)(h >> 32);
    for (int o = 32; o > 0; o >>= 1) {
        lo ^= (unsigned)__shfl_xor((int)lo, o, 64);
        hi ^= (unsigned)__shfl_xor((int)hi, o, 64);
    }
    return (((bb_t)hi << 32) | lo) ^ state_key(p.turn, p.castling, ep_legal ? p.ep : -1);
}

// One ply of a replay from the start position, by a one-wave workgroup: make the move, stage it in LDS, scan hist[0..i] for repetitions,
// merge the flags, store hist[i + 1], fence.  tpos: the chain's tree positions (k_set_position: the slot's; k_encode_positions passes hist).
__device__ inline void replay_step(Position& cur, move_t m, int i, Position* hist, const Position* tpos, Position* s_np, int lane) {
    make_move(cur, m);
    if (lane == 0) *s_np = cur;
    __syncthreads();
    DevChain ch{hist, i, tpos, nullptr, s_np, i + 1};
    uint8_t rf = rep_flags_wave(ch, i + 1, cur.key, lane);
    cur.flags = (uint8_t)((cur.flags & F_IRREV) | rf);
    __syncthreads();
    if (lane == 0) hist[i + 1] = cur;
    __threadfence_block();
    __syncthreads();
}

// Is mv among the generated legal moves s_moves[0 .. nl) (LDS)?  Lane-parallel: rounds of 64 and one ballot; the result is
// wave-uniform.  No barrier in here: the caller orders the list's stores before it and the next generation behind it.
__device__ __forceinline__ bool legal_has_move(const move_t* s_moves, int nl, move_t mv, int lane) {
    bool hit = false;
    for (int k = lane; k < nl; k += 64) hit |= s_moves[k] == mv;
    return __ballot(hit) != 0;
}

// The checked replay of a one-wave workgroup: plays mv[0 .. n) from cur (= hist[0]) into hist[1 ..] with replay_step, every move
// looked up among the legal moves first, and stops in front of the first that is absent.  -> the number of moves played;
// status: 0, or -(i + 1) for an illegal move i.  s_moves [MAXC] and s_np are the caller's LDS.
__device__ inline int replay_checked(Position& cur, const uint16_t* mv, int n, Position* hist, move_t* s_moves, Position* s_np, int lane,
                                     int& status) {
    status = 0;
    for (int i = 0; i < n; i++) {
        int nl = 0;
        gen_legal_wave(cur, s_moves, lane, nl);
        __syncthreads();
        const bool found = legal_has_move(s_moves, nl, mv[i], lane);
        __syncthreads();
        if (!found) {
            status = -(i + 1);
            return i;
        }
        replay_step(cur, mv[i], i, hist, hist, s_np, lane);
    }
    return n;
}

}  // namespace sc
