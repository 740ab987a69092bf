// merge_kernels.hip -- identical training positions merged on the device, targets averaged (sc_merge_positions).
//
// Rows of the compact training tensors (8 548 B per ply) that are the same sample input -- board bytes, meta, n_legal and the
// first n_legal action indices -- become one row with the mean visit shares and the mean outcome.  A key finds the candidates, a
// byte compare decides; every sum runs in ascending position, in float32, without a float atomic.  On `stream`, in this order:
//
//   k_row_key      one wavefront per position: the row's 7 168 board bytes as 16-byte loads (7 per lane, coalesced), meta, n_legal
//       and the action indices below n_legal (the padding is masked away), all issued before the first use (landed()), folded
//       into two 64-bit accumulators per lane -- h = (h ^ w) * K, which depends on the dword's place in the lane, from a seed that
//       depends on the lane -- finished, summed over the wave and masked to key_bits.  Rows outside the source and rows with
//       n_legal outside 0..218 get no key: they are counted and marked (ST_OUTSIDE, ST_BAD_LEGAL).
//   k_find_head    one thread per position: open addressing over >= 2 n_in slots.  A slot is claimed by an integer
//       compare-and-swap of the POSITION (whose key then is the slot's key: no 128-bit atomic is needed), the smallest position of
//       a key is kept with an integer atomicMin.  The probe loop is bounded by the table size; a position that finds no slot
//       becomes a group of its own and is counted as a key clash.  No loop waits for another wave.
//   k_verify       one wavefront per position: byte compare with the row of the key's head.  Equal: a member of that head.
//       Different (a key clash): a group of its own, counted.
//   (scan)         scl::exclusive_scan_u32 (scan_kernels.hip) of the head flags: group numbers ascend with the head's position,
//       and the number of groups is counts[0].
//   k_group        group_of, and the (group, position) pairs of a stable radix sort (rocPRIM, header-only) by group: members of
//       a group in ascending position; thread 0 starts the largest count at 1.  k_segments: where each group starts.
//   k_merge        one wavefront per group: the head's planes, meta, indices copied with 16-byte loads and stores; lane i owns
//       share entries i, i + 64, i + 128, i + 192 and walks the members in order, the loads of 16 members issued before the
//       first of their adds; s / (float) m is the IEEE division (no -ffast-math in this unit; v_div_scale / v_div_fmas /
//       v_div_fixup in the ISA).  A group of one is copied bit for bit.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "launchers.hpp"
#include "wave_util.hpp"

namespace scmg {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));

// the workspace's regions as pointers
struct Ws {
    uint64_t* key;
    int32_t* state;
    int32_t* slot_of;
    int32_t* flag;
    int32_t* gid;
    int32_t* tile_sum;
    uint32_t* grp;
    int32_t* pos;
    uint32_t* grp_sorted;
    int32_t* members;
    int32_t* seg;
    int32_t* aux;
    int32_t* slot_rep;
    int32_t* slot_head;
    uint32_t slot_mask;
};

// every loaded register as an operand of an empty asm statement: the loads are all issued, and have landed, before any
// instruction behind it (batch_kernels.hip, landed)
__device__ __forceinline__ void landed(u4 (&c)[7], u4& l, uint32_t& a, uint32_t& b) {
    asm volatile("" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]), "+v"(c[5]), "+v"(c[6]), "+v"(l), "+v"(a), "+v"(b));
}

__device__ __forceinline__ uint64_t mix64(uint64_t z) {   // splitmix64's finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

constexpr uint64_t K1 = 0x9E3779B97F4A7C15ull, K2 = 0xD6E8FEB86659FD93ull;   // odd: h -> (h ^ w) * K is a bijection of h

__device__ __forceinline__ void fold(uint64_t& h1, uint64_t& h2, uint32_t w) {
    h1 = (h1 ^ w) * K1;
    h2 = (h2 + w) * K2;
    h2 ^= h2 >> 29;
}

// the action indices of chunk `lane` (entries 8 lane .. 8 lane + 7) with the entries from n_legal on cleared
__device__ __forceinline__ u4 legal_masked(u4 v, int lane, int nl) {
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const int e = 8 * lane + 2 * d;
        v[d] &= (e < nl ? 0x0000ffffu : 0u) | (e + 1 < nl ? 0xffff0000u : 0u);
    }
    return v;
}

// the sample-defining bytes of a source row in the registers of one wavefront
struct RowRegs {
    u4 c[7];
    u4 li;
    uint32_t mx;
    uint32_t nl;
};
__device__ __forceinline__ void load_row(const MergeArgs& A, size_t row, int lane, RowRegs& R) {
    const u4* cells = reinterpret_cast<const u4*>(A.boards + row * CELLS);
#pragma unroll
    for (int k = 0; k < 7; k++) R.c[k] = cells[lane + 64 * k];
    R.li = u4{0, 0, 0, 0};
    if (lane < 28) R.li = reinterpret_cast<const u4*>(A.legal_idx + row * LEGAL_ROW)[lane];
    R.mx = lane < META ? (uint32_t)A.meta[row * META + lane] : 0u;
    R.nl = (uint32_t)A.n_legal[row];
}

__global__ __launch_bounds__(256) void k_row_key(MergeArgs A, Ws W) {
    const int lane = threadIdx.x & 63;
    const int p = scw::uniform((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (p >= A.n_in) return;
    const int r = scw::uniform(A.rows ? A.rows[p] : p);
    if (r < 0 || r >= A.n_src) {   // nothing is read through r
        if (lane == 0) {
            W.state[p] = ST_OUTSIDE;
            atomicAdd(W.aux + 1, 1);
            atomicAdd(W.aux + 4, 1);
        }
        return;
    }
    RowRegs R;
    load_row(A, (size_t)r, lane, R);
    landed(R.c, R.li, R.mx, R.nl);
    const int nl = scw::uniform((int)R.nl);
    if (nl < 0 || nl > MAX_LEGAL) {   // the same as nothing: a group of one
        if (lane == 0) {
            W.state[p] = ST_BAD_LEGAL;
            atomicAdd(W.aux + 1, 1);
        }
        return;
    }
    uint64_t h1 = mix64(0x243F6A8885A308D3ull + (uint64_t)(lane + 1) * K1), h2 = mix64(0x13198A2E03707344ull + (uint64_t)(lane + 1) * K2);
#pragma unroll
    for (int k = 0; k < 7; k++)
#pragma unroll
        for (int d = 0; d < 4; d++) fold(h1, h2, R.c[k][d]);
    fold(h1, h2, lane == META ? (uint32_t)nl : R.mx);   // lanes 0..6 meta, lane 7 n_legal, the others 0
    const u4 li = legal_masked(R.li, lane, nl);          // lanes 28.. hold zeros
#pragma unroll
    for (int d = 0; d < 4; d++) fold(h1, h2, li[d]);
    uint64_t lo = mix64(scw::wave_sum_u64(mix64(h1)));
    uint64_t hi = mix64(scw::wave_sum_u64(mix64(h2)) ^ K1);
    const int kb = A.key_bits;
    lo &= kb >= 64 ? ~0ull : ((1ull << kb) - 1);
    hi &= kb <= 64 ? 0ull : kb >= 128 ? ~0ull : ((1ull << (kb - 64)) - 1);
    if (lane == 0) {
        W.key[2 * (size_t)p] = lo;
        W.key[2 * (size_t)p + 1] = hi;
        W.state[p] = ST_OK;
    }
}

__global__ __launch_bounds__(256) void k_find_head(MergeArgs A, Ws W) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= (unsigned)A.n_in || W.state[p] != ST_OK) return;
    const uint64_t lo = W.key[2 * (size_t)p], hi = W.key[2 * (size_t)p + 1];
    uint32_t s = (uint32_t)mix64(lo ^ (hi * K2)) & W.slot_mask;
    int found = -1;
    for (uint32_t t = 0; t <= W.slot_mask; t++, s = (s + 1) & W.slot_mask) {   // bounded by the table
        const int old = atomicCAS(W.slot_rep + s, -1, (int)p);
        if (old == -1 || (W.key[2 * (size_t)old] == lo && W.key[2 * (size_t)old + 1] == hi)) {
            atomicMin(W.slot_head + s, (int)p);
            found = (int)s;
            break;
        }
    }
    W.slot_of[p] = found;   // -1: the table was full (it has twice as many slots as positions) -- k_verify counts it
}

__global__ __launch_bounds__(256) void k_verify(MergeArgs A, Ws W) {
    const int lane = threadIdx.x & 63;
    const int p = scw::uniform((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (p >= A.n_in) return;
    const int st = scw::uniform(W.state[p]);
    int into = p, head_flag = 1, clash = 0;
    if (st == ST_OUTSIDE) {
        into = -1;
        head_flag = 0;
    } else if (st == ST_OK) {
        const int s = scw::uniform(W.slot_of[p]);
        const int h = s < 0 ? p : scw::uniform(W.slot_head[s]);
        if (s < 0) {
            clash = 1;
        } else if (h != p) {   // h < p, a position with the same key whose row is valid
            const int ra = scw::uniform(A.rows ? A.rows[p] : p), rb = scw::uniform(A.rows ? A.rows[h] : h);
            RowRegs Ra, Rb;
            load_row(A, (size_t)ra, lane, Ra);
            load_row(A, (size_t)rb, lane, Rb);
            landed(Ra.c, Ra.li, Ra.mx, Ra.nl);
            landed(Rb.c, Rb.li, Rb.mx, Rb.nl);
            u4 d = legal_masked(Ra.li ^ Rb.li, lane, (int)Ra.nl);
#pragma unroll
            for (int k = 0; k < 7; k++) d |= Ra.c[k] ^ Rb.c[k];
            const uint32_t diff = d.x | d.y | d.z | d.w | (Ra.mx ^ Rb.mx) | (Ra.nl ^ Rb.nl);
            if (__ballot(diff != 0) != 0) clash = 1;
            else {
                into = h;
                head_flag = 0;
            }
        }
    }
    if (lane == 0) {
        W.slot_of[p] = into;
        W.flag[p] = head_flag;
        if (clash) atomicAdd(W.aux + 2, 1);
    }
}

__global__ __launch_bounds__(256) void k_group(MergeArgs A, Ws W) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= (unsigned)A.n_in) return;
    const int into = W.slot_of[p];
    const int g = into < 0 ? -1 : W.gid[into];   // into is a head: gid counts the heads before it
    if (A.group_of) A.group_of[p] = g;
    W.grp[p] = g < 0 ? (uint32_t)A.n_in : (uint32_t)g;
    W.pos[p] = (int)p;
    if (p == 0) W.aux[3] = W.aux[0] > 0 ? 1 : 0;   // the largest m so far: k_merge raises it for every larger group
}

__global__ __launch_bounds__(256) void k_segments(int n, Ws W) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)n) return;
    const uint32_t g = W.grp_sorted[i];
    if (i == 0 || W.grp_sorted[i - 1] != g) W.seg[g] = (int)i;   // g <= n: seg has n + 1 entries
}

struct Shares {
    float x[4];
    float oc;
};
__device__ __forceinline__ void load_shares(const MergeArgs& A, size_t row, int lane, Shares& S) {
    const float* dl = A.dist_legal + row * LEGAL_ROW;
#pragma unroll
    for (int k = 0; k < 3; k++) S.x[k] = dl[lane + 64 * k];
    S.x[3] = lane < LEGAL_ROW - 192 ? dl[lane + 192] : 0.f;
    S.oc = A.outcome[row];
}
__device__ __forceinline__ void shares_landed(Shares& S) {
    asm volatile("" : "+v"(S.x[0]), "+v"(S.x[1]), "+v"(S.x[2]), "+v"(S.x[3]), "+v"(S.oc));
}

constexpr int DEPTH = 16;   // members in flight per wave of k_merge

__global__ __launch_bounds__(256) void k_merge(MergeArgs A, Ws W) {
    const int lane = threadIdx.x & 63;
    const int j = scw::uniform((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const int G = scw::uniform(W.aux[0]);
    if (j >= A.n_in || j >= G) return;
    const int start = scw::uniform(W.seg[j]);
    const int end = j + 1 < G ? scw::uniform(W.seg[j + 1]) : A.n_in - scw::uniform(W.aux[4]);
    const int m = end - start;
    const int p0 = scw::uniform(W.members[start]);   // the smallest position of the group: its head
    const size_t r0 = (size_t)scw::uniform(A.rows ? A.rows[p0] : p0);
    const size_t jj = (size_t)j;
    RowRegs H;
    Shares S;
    load_row(A, r0, lane, H);
    load_shares(A, r0, lane, S);
    landed(H.c, H.li, H.mx, H.nl);
    shares_landed(S);
    if (A.out_boards) {
        u4* ob = reinterpret_cast<u4*>(A.out_boards + jj * CELLS);
#pragma unroll
        for (int k = 0; k < 7; k++) ob[lane + 64 * k] = H.c[k];
    }
    if (A.out_legal_idx && lane < 28) reinterpret_cast<u4*>(A.out_legal_idx + jj * LEGAL_ROW)[lane] = H.li;
    if (A.out_meta && lane < META) A.out_meta[jj * META + lane] = (int32_t)H.mx;
    const int nl = (int)H.nl;
    uint32_t bits[4], oc_bits = __builtin_bit_cast(uint32_t, S.oc);
#pragma unroll
    for (int k = 0; k < 4; k++) bits[k] = __builtin_bit_cast(uint32_t, S.x[k]);
    if (m > 1) {   // (a group of more than one has a valid n_legal)
        float s[4] = {S.x[0], S.x[1], S.x[2], S.x[3]};
        float so = S.oc;
        for (int base = 1; base < m; base += 64) {
            const int cnt = min(64, m - base);
            int myrow = 0;
            if (lane < cnt) {
                const int q = W.members[start + base + lane];
                myrow = A.rows ? A.rows[q] : q;
            }
            // DEPTH members' loads are issued before the first of their adds: a wave that walks a large group (ply 0 of every
            // game) pays one memory latency per DEPTH members, and the adds still run in ascending position
            for (int i0 = 0; i0 < cnt; i0 += DEPTH) {
                Shares sh[DEPTH];
#pragma unroll
                for (int d = 0; d < DEPTH; d++)   // (past the last member: its row once more, loaded and not used)
                    load_shares(A, (size_t)__builtin_amdgcn_readlane(myrow, scw::uniform(min(i0 + d, cnt - 1))), lane, sh[d]);
#pragma unroll
                for (int d = 0; d < DEPTH; d++) shares_landed(sh[d]);
#pragma unroll
                for (int d = 0; d < DEPTH; d++) {
                    if (i0 + d < cnt) {
#pragma unroll
                        for (int k = 0; k < 4; k++) s[k] = s[k] + sh[d].x[k];
                        so = so + sh[d].oc;
                    }
                }
            }
        }
        const float fm = (float)m;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (lane + 64 * k < nl) bits[k] = __builtin_bit_cast(uint32_t, s[k] / fm);
        oc_bits = __builtin_bit_cast(uint32_t, so / fm);
    }
    if (A.out_dist_legal) {
        uint32_t* od = reinterpret_cast<uint32_t*>(A.out_dist_legal + jj * LEGAL_ROW);
#pragma unroll
        for (int k = 0; k < 3; k++) od[lane + 64 * k] = bits[k];
        if (lane < LEGAL_ROW - 192) od[lane + 192] = bits[3];
    }
    if (lane == 0) {
        if (A.out_n_legal) A.out_n_legal[j] = nl;
        if (A.out_outcome) reinterpret_cast<uint32_t*>(A.out_outcome)[j] = oc_bits;
        if (A.out_count) A.out_count[j] = m;
        if (A.out_first) A.out_first[j] = p0;
        // the largest m: groups of one are k_group's business, and a group no larger than what is already there has nothing
        // to add -- one atomic per group on one address would serialise in the L2 and be most of the kernel's time
        if (m > 1 && m > __atomic_load_n(W.aux + 3, __ATOMIC_RELAXED)) atomicMax(W.aux + 3, m);
    }
}

}  // namespace scmg

namespace scl {
hipError_t merge_positions(const scmg::MergeArgs& a, hipStream_t s, const char** why) {
    using namespace scmg;
    *why = nullptr;
    const int n = a.n_in;
    const Workspace L = workspace(n);
    Ws W{};
    W.key = reinterpret_cast<uint64_t*>(a.ws + L.key);
    W.state = reinterpret_cast<int32_t*>(a.ws + L.state);
    W.slot_of = reinterpret_cast<int32_t*>(a.ws + L.slot_of);
    W.flag = reinterpret_cast<int32_t*>(a.ws + L.flag);
    W.gid = reinterpret_cast<int32_t*>(a.ws + L.gid);
    W.tile_sum = reinterpret_cast<int32_t*>(a.ws + L.tile_sum);
    W.grp = reinterpret_cast<uint32_t*>(a.ws + L.grp);
    W.pos = reinterpret_cast<int32_t*>(a.ws + L.pos);
    W.grp_sorted = reinterpret_cast<uint32_t*>(a.ws + L.grp_sorted);
    W.members = reinterpret_cast<int32_t*>(a.ws + L.members);
    W.seg = reinterpret_cast<int32_t*>(a.ws + L.seg);
    W.aux = reinterpret_cast<int32_t*>(a.ws + L.aux);
    W.slot_rep = reinterpret_cast<int32_t*>(a.ws + L.slot_rep);
    W.slot_head = reinterpret_cast<int32_t*>(a.ws + L.slot_head);
    W.slot_mask = L.slots - 1;

    // the sort's keys are group numbers, n for a position in no group: the bits of n
    unsigned bits = 1;
    while (bits < 31 && ((unsigned)n >> bits) != 0) bits++;
    size_t sort_need = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, sort_need, W.grp, W.grp_sorted, W.pos, W.members, (size_t)n, 0u, bits, s, false);
    if (e != hipSuccess) return e;
    if (sort_need > L.sort_bytes) {
        *why = "the radix sort asks for more scratch than sc_merge_positions_workspace reserves for it";
        return hipErrorInvalidValue;
    }

    if ((e = hipMemsetAsync(W.aux, 0, 32, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(W.slot_rep, 0xff, (size_t)L.slots * 4, s)) != hipSuccess) return e;    // -1: free
    if ((e = hipMemsetAsync(W.slot_head, 0x7f, (size_t)L.slots * 4, s)) != hipSuccess) return e;   // above every position
    const unsigned waves = (unsigned)((n + 3) / 4), threads = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_row_key, dim3(waves), dim3(256), 0, s, a, W);
    hipLaunchKernelGGL(k_find_head, dim3(threads), dim3(256), 0, s, a, W);
    hipLaunchKernelGGL(k_verify, dim3(waves), dim3(256), 0, s, a, W);
    // flags are 0 or 1 and group numbers non-negative: the same bits as uint32; the number of groups goes to aux[0]
    exclusive_scan_u32((uint32_t)n, reinterpret_cast<const uint32_t*>(W.flag), reinterpret_cast<uint32_t*>(W.tile_sum),
                       reinterpret_cast<uint32_t*>(W.gid), reinterpret_cast<uint32_t*>(W.aux), s);
    hipLaunchKernelGGL(k_group, dim3(threads), dim3(256), 0, s, a, W);
    size_t sort_bytes = L.sort_bytes;
    e = rocprim::radix_sort_pairs(a.ws + L.sort_tmp, sort_bytes, W.grp, W.grp_sorted, W.pos, W.members, (size_t)n, 0u, bits, s, false);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_segments, dim3(threads), dim3(256), 0, s, n, W);
    hipLaunchKernelGGL(k_merge, dim3(waves), dim3(256), 0, s, a, W);
    if (a.counts && (e = hipMemcpyAsync(a.counts, W.aux, 4 * sizeof(int32_t), hipMemcpyDeviceToDevice, s)) != hipSuccess) return e;
    return hipGetLastError();
}
}  // namespace scl
