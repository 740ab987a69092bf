// nn_kernels.hip -- the network's kernels (tower, value_head.ffn.0, value tail) and their launchers.  Contraction on: search_select.hpp.
#include "nn_kernels.hpp"
#include "nn_tower32.hpp"
#include "tower_config.hpp"

namespace scnn {

template <class P, int C, int RS, int TPI, int AB = SC_T32_AB>
__global__ __launch_bounds__(256, 1) void k_tower32(TowerArgs A) {
    if ((int)blockIdx.x >= A.n_pos) return;
    NoHand nh;
    tower_body<P, C, RS, TPI, AB>(A, (int)blockIdx.x, nullptr, NoPre(), nh);
}

// grid = (ceil(n/64), KSPLIT)
__global__ __launch_bounds__(256) void k_value_fc1(Fc1Args A) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int mb = blockIdx.x, ks = blockIdx.y;
    __shared__ __attribute__((aligned(16))) bf16_t s_a[FC1_TILE_LDS / 2];
    Fc1W w;
    fc1_wload(w, A.net, ks, A.ksplit, wave, lane);
    fc1_stage_a(s_a, A.hval, A.n_pos, mb, ks, A.ksplit, tid);
    __syncthreads();   // A tile staged
    fc1_mma_store(w, s_a, A.vpart, A.n_pos, mb, ks, A.ksplit, wave, lane);
}

// value head tail (py/module.py:95-106,147-149), one wave per position: the arithmetic is value_tail.hpp's, shared with the
// search kernel's fused tail (search_expand.hpp: value_tail_issue / value_tail_finish), so `predict` and the value the
// search backs up are the same bits.
__global__ __launch_bounds__(64) void k_value_finish(VfinArgs A) {
    const int pos = blockIdx.x, lane = threadIdx.x;
    if (pos >= A.n_pos) return;
    const float* wf = A.net.wf;
    scvt::ValueTail t;
#pragma unroll
    for (int k = 0; k < 7; k++) t.meta[k] = A.meta[(size_t)pos * A.meta_stride + k];
    const int j = 2 * lane;   // lane owns output columns 2*lane, 2*lane+1
    const float* vp = A.vpart + (size_t)pos * FC1_N + j;
    const size_t vstride = (size_t)A.n_pos * FC1_N;
#pragma unroll
    for (int ks = 0; ks < 32; ks++) t.acc[ks] = *reinterpret_cast<const float2*>(vp + (size_t)ks * vstride);
    if (A.ksplit > 32) {
#pragma unroll
        for (int ks = 32; ks < 64; ks++) t.acc[ks] = *reinterpret_cast<const float2*>(vp + (size_t)ks * vstride);
    } else {
#pragma unroll
        for (int ks = 32; ks < 64; ks++) t.acc[ks] = make_float2(0.f, 0.f);
    }
    t.bias = *reinterpret_cast<const float2*>(wf + A.net.f_fc1b + j);
    t.w2 = *reinterpret_cast<const float2*>(wf + A.net.f_fc2w + j);
#pragma unroll
    for (int k = 0; k < 7; k++) t.wm[k] = *reinterpret_cast<const float2*>(wf + A.net.f_fc1m + k * FC1_N + j);
    t.fc2b = wf[A.net.f_fc2b];
    const float v = scvt::value_tail_compute(t, A.ksplit);
    if (lane == 0) A.value[pos] = v;
}

}  // namespace scnn

#include "launchers.hpp"

namespace scl {
// One instantiation of the channel-major tower (nn_tower32.hpp) per precision and trunk width: tower_config.hpp.
template <class T>
constexpr auto tower_kernel(T) { return &scnn::k_tower32<typename T::P, T::C, T::RS, T::TPI, T::AB>; }

const char* nn_init() {
    for (bool fp8 : {false, true})
        for (int C : {128, 256}) {
            const hipError_t e = scnn::with_tower_cfg(fp8, C, [](auto cfg) {
                return hipFuncSetAttribute(reinterpret_cast<const void*>(tower_kernel(cfg)), hipFuncAttributeMaxDynamicSharedMemorySize, cfg.LDS_BYTES);
            });
            if (e != hipSuccess) return hipGetErrorString(e);
        }
    return nullptr;
}
void tower(const scnn::TowerArgs& a, hipStream_t s) {
    if (a.n_pos <= 0) return;
    scnn::with_tower_cfg(a.net.fp8, a.net.C, [&](auto cfg) { hipLaunchKernelGGL(tower_kernel(cfg), dim3(a.n_pos), dim3(256), cfg.LDS_BYTES, s, a); });
}
void value_fc1(const scnn::Fc1Args& a, hipStream_t s) {
    if (a.n_pos <= 0 || a.ksplit < 64 || scnn::FC1_K % (a.ksplit * 32)) return;   // the kernel's LDS tile holds K / 64 columns
    hipLaunchKernelGGL(scnn::k_value_fc1, dim3((a.n_pos + 63) / 64, a.ksplit), dim3(256), 0, s, a);
}
void value_finish(const scnn::VfinArgs& a, hipStream_t s) {
    if (a.n_pos <= 0) return;
    hipLaunchKernelGGL(scnn::k_value_finish, dim3(a.n_pos), dim3(64), 0, s, a);
}
}  // namespace scl
