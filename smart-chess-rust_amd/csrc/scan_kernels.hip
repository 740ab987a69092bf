// scan_kernels.hip -- the exclusive scan of uint32 counts on the device (scl::exclusive_scan_u32): perft's move counts into child
// slots, the merge's head flags into group numbers.
//
// Tiles of SCAN_TILE = 1 024 counts, one workgroup of 256 threads each, four counts per thread; sums wrap modulo 2^32.
//
//   k_scan_tiles   the total of every tile.
//   k_scan_sums    ONE workgroup: the exclusive scan of the tile totals in place, 256 of them at a time with the carry of the ones
//       before; the carry behind the last is the total.
//   k_scan_apply   the scan inside every tile, on top of the tile's carry.
#include <hip/hip_runtime.h>

#include "launchers.hpp"

namespace scsn {

using scl::SCAN_TILE;

__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* s_buf, uint32_t* total) {   // 256 threads
    const int t = threadIdx.x;
    s_buf[t] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const uint32_t x = t >= o ? s_buf[t - o] : 0u;
        __syncthreads();
        s_buf[t] += x;
        __syncthreads();
    }
    const uint32_t incl = s_buf[t];
    *total = s_buf[255];
    __syncthreads();
    return incl - v;
}
__device__ __forceinline__ uint32_t tile_counts(const uint32_t* cnt, uint32_t n, uint32_t base, uint32_t f[4]) {
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        f[k] = base + k < n ? cnt[base + k] : 0u;
        sum += f[k];
    }
    return sum;
}
__global__ __launch_bounds__(256) void k_scan_tiles(uint32_t n, const uint32_t* cnt, uint32_t* tile_sum) {
    __shared__ uint32_t s_buf[256];
    uint32_t f[4], total;
    const uint32_t v = tile_counts(cnt, n, blockIdx.x * (uint32_t)SCAN_TILE + threadIdx.x * 4u, f);
    block_excl_scan(v, s_buf, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}
__global__ __launch_bounds__(256) void k_scan_sums(uint32_t n_tiles, uint32_t* tile_sum, uint32_t* total_out) {   // one workgroup
    __shared__ uint32_t s_buf[256];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_tiles; base += 256) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n_tiles ? tile_sum[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_excl_scan(v, s_buf, &total);
        if (i < n_tiles) tile_sum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}
__global__ __launch_bounds__(256) void k_scan_apply(uint32_t n, const uint32_t* cnt, const uint32_t* tile_sum, uint32_t* off) {
    __shared__ uint32_t s_buf[256];
    uint32_t f[4], total;
    const uint32_t base = blockIdx.x * (uint32_t)SCAN_TILE + threadIdx.x * 4u;
    const uint32_t v = tile_counts(cnt, n, base, f);
    uint32_t at = tile_sum[blockIdx.x] + block_excl_scan(v, s_buf, &total);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (base + k < n) off[base + k] = at;
        at += f[k];
    }
}

}  // namespace scsn

namespace scl {
void exclusive_scan_u32(uint32_t n, const uint32_t* d_in, uint32_t* d_tile_sum, uint32_t* d_out, uint32_t* d_total, hipStream_t s) {
    if (n == 0) return;
    const unsigned tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    hipLaunchKernelGGL(scsn::k_scan_tiles, dim3(tiles), dim3(256), 0, s, n, d_in, d_tile_sum);
    hipLaunchKernelGGL(scsn::k_scan_sums, dim3(1), dim3(256), 0, s, tiles, d_tile_sum, d_total);
    hipLaunchKernelGGL(scsn::k_scan_apply, dim3(tiles), dim3(256), 0, s, n, d_in, d_tile_sum, d_out);
}
}  // namespace scl
