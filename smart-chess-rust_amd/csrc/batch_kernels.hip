// batch_kernels.hip -- training minibatches from the compact tensors (sc_gather_batch).
//
// Replaces, for positions already in device memory, the per-sample work of the reference's DataLoader over ChessDataset
// (py/dataset.py:31-44 _prepare, :61-62 the mirrored outcome; scripts/train.py:331-353): sample b of a batch is row rows[b] of
// the tensors layout 0 of sc_encode_steps_device / sc_selfplay_encode_traces leaves behind (8 548 B per ply), widened to the
// trainer's float32 planes [112][8][8], meta [7], dense dist [4672] and outcome (47 392 B) in one pass.
//
//   k_gather_batch   one 256-thread workgroup per sample; the row index is read through a scalar load and is the same in
//       every lane.  Loads: the 7 168 plane bytes are 448 16-byte chunks (thread t takes chunk t, waves 0..2 also chunk t + 256);
//       wave 3 takes the sparse rows instead -- lane e < 28 the 16 bytes of action indices 8e .. 8e+7 and the two 16-byte chunks
//       of their shares.  All of a thread's loads are issued before the first use (landed() below; checked in the ISA).
//       Planes: a chunk is 16 planes of one square; it is written to LDS with a square stride of 29 dwords (116 B).  Thread
//       (pg, q) then reads the dword of planes 4pg..4pg+3 of squares 4q..4q+3 -- within a wavefront 4 values of pg and 16 of q,
//       bank (4q * 29 + pg) mod 64 = (52 q + pg) mod 64: 64 distinct banks (a stride of 28 dwords would fold them onto 16) -- and
//       stores four 16-byte pieces, one per plane; the 16 lanes of one pg write a plane's 256 contiguous bytes.
//       dist: the row is built in LDS (zero, barrier, <= 218 stores by wave 3, barrier) and streamed out, 1 168 16-byte stores:
//       no global address is written twice by a launch.  Only entries i < n_legal are looked at: the padding points at action 0,
//       which can be a legal move.
//       The mirror changes meta and the outcome only (encode_kernels.hip, k_steps_dist: Board::rotate()'s meta).
//   Bad input is contained on the device: a row index outside [0, n_src) reads nothing and leaves NaN in all four outputs of
//   the sample; n_legal outside 0..218 or an action index >= 4672 among the legal ones stores nothing through it and leaves NaN
//   in the sample's dist row.  Each adds 1 to n_bad[0] (one integer atomic per bad sample).
#include <hip/hip_runtime.h>

#include "launchers.hpp"

namespace scbt {

constexpr int SQ_STRIDE = 29;   // dwords per square in LDS: 28 of planes + 1 (odd: lane = square walks all 64 banks)

__device__ __forceinline__ float quiet_nan() { return __builtin_bit_cast(float, 0x7fc00000u); }
__device__ __forceinline__ float byte_f(uint32_t w, int k) { return (float)(int8_t)((w >> (8 * k)) & 0xffu); }   // signed, exact

// an empty asm statement that takes every loaded register as an operand: the loads handed to it are all issued, and have
// landed, before any instruction behind it (score_kernels.hip, rows_landed)
typedef uint32_t u4 __attribute__((ext_vector_type(4)));
// (m: the mirror byte, whose address is the same in every lane -- without this the compiler waits for it, to hold it in a scalar
// register, before the first 16-byte load is out)
__device__ __forceinline__ void landed(u4& a, u4& b, uint32_t& m) { asm volatile("" : "+v"(a), "+v"(b), "+v"(m)); }
__device__ __forceinline__ void landed(u4& a, u4& b, u4& c, u4& d, uint32_t& m) {
    asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(m));
}
__device__ __forceinline__ float4 nan4() { return make_float4(quiet_nan(), quiet_nan(), quiet_nan(), quiet_nan()); }

__device__ __forceinline__ void stage_cell(uint32_t* s_pl, int chunk, const u4& v) {
    uint32_t* d = s_pl + (chunk / 7) * SQ_STRIDE + (chunk % 7) * 4;   // square chunk / 7, planes 16 (chunk % 7) ..
    d[0] = v.x;
    d[1] = v.y;
    d[2] = v.z;
    d[3] = v.w;
}

// planes 4pg .. 4pg+3 of squares 4q .. 4q+3 -> four 16-byte stores
__device__ __forceinline__ void planes_out(const uint32_t* s_pl, int task, float* out) {
    const int pg = task >> 4, q = task & 15;
    uint32_t w[4];
#pragma unroll
    for (int s = 0; s < 4; s++) w[s] = s_pl[(4 * q + s) * SQ_STRIDE + pg];
#pragma unroll
    for (int k = 0; k < 4; k++)
        *reinterpret_cast<float4*>(out + (4 * pg + k) * 64 + 4 * q) = make_float4(byte_f(w[0], k), byte_f(w[1], k), byte_f(w[2], k), byte_f(w[3], k));
}

__global__ __launch_bounds__(256) void k_gather_batch(GatherArgs A) {
    __shared__ __attribute__((aligned(16))) float s_dist[ROW];
    __shared__ uint32_t s_pl[64 * SQ_STRIDE];
    __shared__ int s_oob;
    const int t = threadIdx.x;
    const size_t b = blockIdx.x;
    const int r = A.rows[b];
    float* ob = A.out_boards ? A.out_boards + b * CELLS : nullptr;
    float4* od = A.out_dist ? reinterpret_cast<float4*>(A.out_dist + b * ROW) : nullptr;
    if (r < 0 || r >= A.n_src) {   // the same in every lane: nothing is read through r
        if (ob)
            for (int i = t; i < CELLS / 4; i += 256) reinterpret_cast<float4*>(ob)[i] = nan4();
        if (od)
            for (int i = t; i < ROW4; i += 256) od[i] = nan4();
        if (A.out_meta && t < 7) A.out_meta[b * 7 + t] = quiet_nan();
        if (t == 0) {
            if (A.out_outcome) A.out_outcome[b] = quiet_nan();
            if (A.n_bad) atomicAdd(A.n_bad, 1);
        }
        return;
    }
    const size_t row = (size_t)r;
    // ---- every load of the sample, then the first use.  The small rows first: their addresses are the same in every lane
    // (scalar loads but for the mirror byte and the lanes' meta entries), nothing waits for them before the 16-byte loads are out
    uint32_t mb = A.mirror ? A.mirror[b] : 0;
    const int32_t nl = A.n_legal[row];
    const float oc = A.outcome[row];
    const int32_t* m = A.meta + row * 7;
    const int32_t m0 = m[0];
    int32_t ma = 0, mr = 0;
    if (t < 7) {
        ma = m[t];
        mr = m[t >= 2 && t <= 5 ? t ^ 6 : t];   // Board::rotate() exchanges the castling rights: 2 <-> 4, 3 <-> 5
    }
    const u4* cells = reinterpret_cast<const u4*>(A.boards + row * CELLS);
    const bool sparse_wave = __builtin_amdgcn_readfirstlane(t >> 6) == 3;   // a scalar branch: wave 3
    const int e = t - 192 < 28 ? t - 192 : 27;     // its lanes past 27 ask for lane 27's chunks again and do not use them
    u4 c0 = cells[t], c1, d0 = {0, 0, 0, 0}, d1 = {0, 0, 0, 0};
    if (sparse_wave) {
        c1 = reinterpret_cast<const u4*>(A.legal_idx + row * LEGAL_ROW)[e];
        const u4* dl = reinterpret_cast<const u4*>(A.dist_legal + row * LEGAL_ROW);
        d0 = dl[2 * e];
        d1 = dl[2 * e + 1];
        landed(c0, c1, d0, d1, mb);
    } else {
        c1 = cells[t + 256];
        landed(c0, c1, mb);
    }

    if (ob) {
        stage_cell(s_pl, t, c0);
        if (!sparse_wave) stage_cell(s_pl, t + 256, c1);
    }
    if (od)
        for (int i = t; i < ROW4; i += 256) reinterpret_cast<float4*>(s_dist)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t == 0) s_oob = 0;
    __syncthreads();
    const bool mir = mb != 0;
    const bool nl_ok = nl >= 0 && nl <= MAX_LEGAL;
    if (sparse_wave && t - 192 < 28) {
        const int lim = nl_ok ? nl : 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (8 * e + j < lim) {
                const uint32_t idx = (c1[j >> 1] >> (16 * (j & 1))) & 0xffffu;
                if (idx >= (uint32_t)ROW) s_oob = 1;
                else if (od) s_dist[idx] = __builtin_bit_cast(float, j < 4 ? d0[j & 3] : d1[j & 3]);
            }
        }
    }
    if (ob) {
        planes_out(s_pl, t, ob);
        if (t < 192) planes_out(s_pl, t + 256, ob);
    }
    if (A.out_meta && t < 7) {
        // Board::rotate(): [1 - turn, fullmove + (turn == White), K(opp), Q(opp), K(mover), Q(mover), halfmove]
        const int32_t v = !mir ? ma : t == 0 ? 1 - m0 : t == 1 ? ma + (m0 == 1 ? 1 : 0) : mr;
        A.out_meta[b * 7 + t] = (float)v;
    }
    if (A.out_outcome && t == 0) A.out_outcome[b] = mir ? -oc : oc;
    __syncthreads();
    const bool bad = !nl_ok || s_oob != 0;
    if (od)
        for (int i = t; i < ROW4; i += 256) od[i] = bad ? nan4() : reinterpret_cast<const float4*>(s_dist)[i];
    if (bad && t == 0 && A.n_bad) atomicAdd(A.n_bad, 1);
}

}  // namespace scbt

namespace scl {
void gather_batch(const scbt::GatherArgs& a, hipStream_t s) {
    if (a.n_batch <= 0) return;
    hipLaunchKernelGGL(scbt::k_gather_batch, dim3(a.n_batch), dim3(256), 0, s, a);
}
}  // namespace scl
