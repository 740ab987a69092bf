// score_kernels.hip -- judging a network on recorded positions (sc_score_positions, sc_compare_engines): per-position losses
// and agreement figures from the log-probability rows the tower has just written, and their summaries.
//
// Replaces, for positions already in device memory, the arithmetic of the reference's scripts/train.py validation_step
// (compute_loss1 / compute_loss2, pi_entropy) and scripts/validate_model.py (total variation, |value1 - value2|).
//
// The tower, value_fc1 and value_finish are launched unchanged (device_calls.hip); these kernels only READ what they wrote.
//
//   k_score / k_compare   one wavefront per position (four positions per workgroup).  A row is 4672 floats = 1168 16-byte
//       loads: lane l takes chunks l, l + 64, ..., l + 64 * 18 (the last index clamped to the row and masked in the arithmetic, so
//       no load is guarded), all issued before the first use (rows_landed() below; checked in the ISA: 38 global_load_dwordx4, then
//       the first s_waitcnt vmcnt, in k_score and in k_compare).  Every sum over the row is the same tree: the four floats of a
//       chunk pairwise (2 levels), the lane's 19 chunks pairwise (5 levels), wave_sum_fixed (4 DPP levels + 2) -- 13 additions deep,
//       in a fixed order, so a position's result depends on nothing but its own rows.  The exponential is expf (HIP's
//       math-function table: 1 ulp), the translation unit is compiled with -ffp-contract=off: products are rounded before they are
//       added.  The sparse form of ce is one gather of <= 218 log-probabilities (lane = legal move, four rounds).
//       One kernel serves both dist forms, with the choice made at run time: ent, se and value come from the same instructions
//       whichever form is given (nn_tower32.hpp records what two compilations of "the same" arithmetic did to the priors).
//   k_summary             one workgroup reduces the [P] per-position floats to the summary in double precision: thread t adds
//       entries t, t + 1024, ... in order, then a tree over the 1024 partials in LDS.  No atomics anywhere: two identical calls
//       give bit-identical summaries.
#include "wave_util.hpp"   // wave_sum_fixed (DPP + readlane, fixed order)
#include "launchers.hpp"
#include "score_types.hpp"

namespace scsc {

using scw::wave_sum_fixed;

__device__ __forceinline__ float sum4(float4 t) { return (t.x + t.y) + (t.z + t.w); }
// pairwise over the lane's 19 chunk sums: ((0..4) + (5..9)) + ((10..14) + (15..18)), 5 levels
template <int N>
__device__ __forceinline__ float tree(const float* v) {
    if constexpr (N == 1) {
        return v[0];
    } else {
        constexpr int H = (N + 1) / 2;
        return tree<H>(v) + tree<N - H>(v + H);
    }
}
__device__ __forceinline__ bool finite_f(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ float quiet_nan() { return __builtin_bit_cast(float, 0x7fc00000u); }

// the lane's 19 chunks of a row; chunk 18 exists for lanes 0..15 only: the others re-read the row's last chunk and mask it
__device__ __forceinline__ void load_row(const float* row, int lane, float4 (&r)[19]) {
    const float4* p = reinterpret_cast<const float4*>(row);
#pragma unroll
    for (int j = 0; j < 18; j++) r[j] = p[lane + 64 * j];
    r[18] = p[lane < 16 ? lane + 64 * 18 : ROW4 - 1];
}

__device__ __forceinline__ float ce_term(float d, float lp) { return d != 0.f ? d * lp : 0.f; }   // 0 * logp is never formed
__device__ __forceinline__ float ent_term(float lp) { return expf(lp) * lp; }
__device__ __forceinline__ float tv_term(float a, float b) { return fabsf(expf(a) - expf(b)); }

// Register budget: two rows in flight are 152 VGPRs of load destinations, so the kernels ask for at most two waves per SIMD (256
// VGPRs each) instead of the four the default heuristic aims for -- with four the compiler fetched the second row two chunks at a
// time behind the arithmetic.  rows_landed() pins the order: an empty asm statement that takes every chunk of a row as a register
// operand, so every load of the rows handed to it is issued, and has landed, before any instruction behind it (one s_waitcnt for
// the row instead of one per chunk: the kernels wait for memory, not for issue slots).  Ten operands per statement: the limit is 30.
__device__ __forceinline__ void rows_landed(float4 (&r)[19]) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    f4* v = reinterpret_cast<f4*>(r);
    asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]), "+v"(v[8]), "+v"(v[9]));
    asm volatile("" : "+v"(v[10]), "+v"(v[11]), "+v"(v[12]), "+v"(v[13]), "+v"(v[14]), "+v"(v[15]), "+v"(v[16]), "+v"(v[17]), "+v"(v[18]));
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_score(ScoreArgs A) {
    const int lane = threadIdx.x & 63;
    const int pos = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (pos >= A.n) return;   // wave-uniform
    const float* lrow = A.logp + (size_t)pos * ROW;
    const bool last = lane < 16;
    // Both rows are requested before the choice of the dist form is looked at: behind a branch the compiler held the second row's
    // loads back until most of the first had landed (two round trips in a row).  The sparse form has no second row; its lanes ask
    // for the chunks of the log-probability row again: the same 64-byte lines, requested a moment earlier.
    float4 l[19], d[19];
    load_row(lrow, lane, l);
    load_row(A.dist ? A.dist + (size_t)pos * ROW : lrow, lane, d);
    rows_landed(d);   // 38 loads out, nothing used yet (loads return in order: with d, l has landed too)
    float ce;
    if (A.dist) {
        float t[19];
#pragma unroll
        for (int j = 0; j < 19; j++) {
            float4 q;
            q.x = ce_term(d[j].x, l[j].x);
            q.y = ce_term(d[j].y, l[j].y);
            q.z = ce_term(d[j].z, l[j].z);
            q.w = ce_term(d[j].w, l[j].w);
            t[j] = sum4(q);
        }
        if (!last) t[18] = 0.f;
        ce = -wave_sum_fixed(tree<19>(t));
    } else {
        // lane = legal move i (+ 64 per round); entries at and past n_legal are padding (action 0, share 0) and are not read
        const int nl = A.n_legal[pos];
        const bool bad = nl < 0 || nl > MAX_LEGAL;
        const uint16_t* li = A.legal_idx + (size_t)pos * LEGAL_ROW;
        const float* dl = A.dist_legal + (size_t)pos * LEGAL_ROW;
        float t[4];
        bool oob = false;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int i = lane + 64 * r;
            const bool on = !bad && i < nl;
            const int idx = on ? (int)li[i] : 0;
            const float d = on ? dl[i] : 0.f;
            const bool in = idx < ROW;
            oob |= !in;
            t[r] = (on && in && d != 0.f) ? d * lrow[idx] : 0.f;
        }
        ce = -wave_sum_fixed((t[0] + t[1]) + (t[2] + t[3]));
        // n_legal outside 0..218 or an action index outside the row: nothing was read through them, the position counts as non-finite
        if (bad || __builtin_amdgcn_ballot_w64(oob) != 0) ce = quiet_nan();
    }
    float t[19];
#pragma unroll
    for (int j = 0; j < 19; j++) {
        float4 q;
        q.x = ent_term(l[j].x);
        q.y = ent_term(l[j].y);
        q.z = ent_term(l[j].z);
        q.w = ent_term(l[j].w);
        t[j] = sum4(q);
    }
    if (!last) t[18] = 0.f;
    const float ent = -wave_sum_fixed(tree<19>(t));
    if (lane == 0) {
        const float v = A.value[pos];
        const float dv = v - A.outcome[pos];
        A.ce[pos] = ce;
        A.se[pos] = dv * dv;
        A.ent[pos] = ent;
        if (A.value_out) A.value_out[pos] = v;
    }
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_compare(CompareArgs A) {
    const int lane = threadIdx.x & 63;
    const int pos = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (pos >= A.n) return;
    const bool last = lane < 16;
    float4 a[19], b[19];
    load_row(A.logp1 + (size_t)pos * ROW, lane, a);
    load_row(A.logp2 + (size_t)pos * ROW, lane, b);
    rows_landed(a);
    rows_landed(b);
    float t[19];
#pragma unroll
    for (int j = 0; j < 19; j++) {
        float4 q;
        q.x = tv_term(a[j].x, b[j].x);
        q.y = tv_term(a[j].y, b[j].y);
        q.z = tv_term(a[j].z, b[j].z);
        q.w = tv_term(a[j].w, b[j].w);
        t[j] = sum4(q);
    }
    if (!last) t[18] = 0.f;
    const float tv = 0.5f * wave_sum_fixed(tree<19>(t));
    if (lane == 0) {
        A.tv[pos] = tv;
        A.dv[pos] = fabsf(A.value1[pos] - A.value2[pos]);
    }
}

// ---- [P] -> summary
constexpr int SUM_T = 1024;

__device__ __forceinline__ double block_sum(double v, double* s) {
    const int t = threadIdx.x;
    __syncthreads();   // (s is reused from one reduction to the next)
    s[t] = v;
    __syncthreads();
    for (int h = SUM_T / 2; h > 0; h >>= 1) {
        if (t < h) s[t] += s[t + h];
        __syncthreads();
    }
    return s[0];
}
__device__ __forceinline__ double block_max(double v, double* s) {
    const int t = threadIdx.x;
    __syncthreads();
    s[t] = v;
    __syncthreads();
    for (int h = SUM_T / 2; h > 0; h >>= 1) {
        if (t < h) s[t] = s[t] > s[t + h] ? s[t] : s[t + h];
        __syncthreads();
    }
    return s[0];
}

// mean, population standard deviation (two passes, as numpy's), max, min of x[0..n) -> out[0..4); a NaN anywhere makes all four NaN
__device__ void stats4(const float* x, int n, double* s, double* out) {
    const int t = threadIdx.x;
    double sum = 0.0, mx = -__builtin_huge_val(), mn = __builtin_huge_val(), nan = 0.0;
    for (int i = t; i < n; i += SUM_T) {
        const double v = (double)x[i];
        sum += v;
        if (v != v) nan = 1.0;
        else {
            mx = v > mx ? v : mx;
            mn = v < mn ? v : mn;
        }
    }
    const double mean = block_sum(sum, s) / (double)n;
    const double gmx = block_max(mx, s), gmn = -block_max(-mn, s), gnan = block_max(nan, s);
    double sq = 0.0;
    for (int i = t; i < n; i += SUM_T) {
        const double dlt = (double)x[i] - mean;
        sq += dlt * dlt;
    }
    const double var = block_sum(sq, s) / (double)n;
    if (t == 0) {
        const double qn = __builtin_nan("");
        out[0] = mean;
        out[1] = sqrt(var);
        out[2] = gnan != 0.0 ? qn : gmx;
        out[3] = gnan != 0.0 ? qn : gmn;
    }
}

__global__ __launch_bounds__(SUM_T) void k_summary(SummaryArgs A) {
    __shared__ double s[SUM_T];
    const int t = threadIdx.x;
    if (A.mode == 0) {
        double c = 0.0, e = 0.0, h = 0.0, bad = 0.0;
        for (int i = t; i < A.n; i += SUM_T) {
            const float ce = A.x0[i], se = A.x1[i], en = A.x2[i];
            c += (double)ce;
            e += (double)se;
            h += (double)en;
            if (!(finite_f(ce) && finite_f(se) && finite_f(en))) bad += 1.0;
        }
        const double sc = block_sum(c, s), se = block_sum(e, s), sh = block_sum(h, s), sb = block_sum(bad, s);
        if (t == 0) {
            A.out[0] = (double)A.n;
            A.out[1] = sc / (double)A.n;
            A.out[2] = se / (double)A.n;
            A.out[3] = sh / (double)A.n;
            A.out[4] = sb;
        }
    } else {
        if (t == 0) A.out[0] = (double)A.n;
        stats4(A.x0, A.n, s, A.out + 1);
        stats4(A.x1, A.n, s, A.out + 5);
    }
}

}  // namespace scsc

namespace scl {
void score_positions(const scsc::ScoreArgs& a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(scsc::k_score, dim3((a.n + 3) / 4), dim3(256), 0, s, a);
}
void compare_rows(const scsc::CompareArgs& a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(scsc::k_compare, dim3((a.n + 3) / 4), dim3(256), 0, s, a);
}
void score_summary(const scsc::SummaryArgs& a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(scsc::k_summary, dim3(1), dim3(scsc::SUM_T), 0, s, a);
}
}  // namespace scl
