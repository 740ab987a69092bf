// wave_util.hpp -- cross-lane helpers of one 64-lane wavefront, one definition each: for the search, the rules, the network, the scoring.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace scw {

// Reductions on latency chains (a tree level of the descent, the softmax, the value tail): four DPP steps inside each row of 16 lanes
// (quad_perm, row_half_mirror, row_mirror: plain VALU moves) and four readlanes to the scalar unit, instead of six dependent trips
// through the LDS crossbar (ds_bpermute).  Fixed order, so results are reproducible; the result is wave-uniform.
template <int CTRL>
__device__ __forceinline__ int dpp_i(int x) { return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xf, 0xf, false); }
template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) { return __builtin_bit_cast(float, dpp_i<CTRL>(__builtin_bit_cast(int, x))); }
__device__ __forceinline__ float readlane_f(float x, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), l)); }
__device__ __forceinline__ int wave_sum_i(int v) {
    v += dpp_i<0xB1>(v);    // quad_perm [1,0,3,2]
    v += dpp_i<0x4E>(v);    // quad_perm [2,3,0,1]
    v += dpp_i<0x141>(v);   // row_half_mirror
    v += dpp_i<0x140>(v);   // row_mirror
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
           __builtin_amdgcn_readlane(v, 48);
}
// (contraction off in the body: inlined into a contracting unit, a caller's multiply must not fuse into the first add)
__device__ __forceinline__ float wave_sum_fixed(float v) {
#pragma clang fp contract(off)
    v += dpp_f<0xB1>(v);
    v += dpp_f<0x4E>(v);
    v += dpp_f<0x141>(v);
    v += dpp_f<0x140>(v);
    return (readlane_f(v, 0) + readlane_f(v, 16)) + (readlane_f(v, 32) + readlane_f(v, 48));
}
__device__ __forceinline__ float wave_max_fixed(float v) {
    v = fmaxf(v, dpp_f<0xB1>(v));
    v = fmaxf(v, dpp_f<0x4E>(v));
    v = fmaxf(v, dpp_f<0x141>(v));
    v = fmaxf(v, dpp_f<0x140>(v));
    return fmaxf(fmaxf(readlane_f(v, 0), readlane_f(v, 16)), fmaxf(readlane_f(v, 32), readlane_f(v, 48)));
}
// butterfly sums (off the hot path), the result in every lane
__device__ inline float wave_sum_f(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline unsigned long long wave_sum_u64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// ... and the butterfly maximum: an arg-max over packed keys (value << 32 | tie-break), the result in every lane
__device__ inline unsigned long long wave_max_u64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long x = __shfl_xor(v, o, 64);
        v = x > v ? x : v;
    }
    return v;
}

// the exclusive prefix sum of v over the lanes of the wave (off the hot path, every lane active); *total = the wave's sum
__device__ inline uint32_t wave_excl_scan_u32(uint32_t v, uint32_t* total) {
    const int lane = (int)(threadIdx.x & 63u);
    uint32_t incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t x = __shfl_up(incl, o, 64);
        if (lane >= o) incl += x;
    }
    *total = __shfl(incl, 63, 64);
    return incl - v;
}

// Synchronisation inside the search functions (dev_expand, dev_select, finish_game): each game is searched by ONE wavefront -- the whole
// workgroup of k_mcts, or wave 0 of the tower's workgroup in the fused step kernel (k_step), where a workgroup barrier would wait for
// waves that never come.  A wave's LDS and vector-memory operations take effect in program order; what is needed between a store by one
// lane and a load by another is that the compiler keeps that order and the operations have completed: a workgroup-scope fence
// (s_waitcnt) plus a wave barrier (scheduling only).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// Promote a wave-uniform value to SGPRs.  All lanes of a game's wave run the scalar chess logic on identical data; telling the compiler
// so (readfirstlane) moves that logic -- 64-bit bitboard arithmetic, bit scans, bit reversal, loop control -- from the vector ALU (2 x
// 32-bit ops, exec-mask branches) onto the scalar unit.
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t uniform(uint64_t v) {
    unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}
// ... and the value lane `sel` holds (sel wave-uniform), in every lane
__device__ __forceinline__ uint64_t from_lane(uint64_t v, int sel) {
    unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, sel);
    unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), sel);
    return ((uint64_t)hi << 32) | lo;
}

}  // namespace scw
