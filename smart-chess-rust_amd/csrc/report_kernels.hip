// report_kernels.hip -- the search report (sc_selfplay_report; the contract is include/sc_engine.h's): ranked lines and principal
// variations read from the slots' trees where they lie.  Compiled with -ffp-contract=off like the other search units (the kernel
// copies the statistics, it computes no value from them).
//
// ONE wavefront (a workgroup of 64 threads) serves one (entry, line) pair, lane = child, in rounds of 64 children: four rounds at
// most (224 children).  Every wave of an entry ranks the root's children itself -- child i has rank #{ j : N[j] > N[i], or
// N[j] == N[i] and j < i }: visits descending, then the generator's order, so rank 0 is the first most-visited child (mcts::step,
// src/mcts.rs:309-311) -- and wave r walks the variation of the child of rank r: to the most-visited child, ties to the lowest
// index, while the node is expanded, has children and the most-visited one has been visited.  Wave 0 also writes the slot's record.
// The kernel runs on the handle's stream behind its completed work, reads N, W, P, MV, H, the control block and the root's history
// record, and stores only into the report buffer: nothing the search reads changes.
#include <hip/hip_runtime.h>

#include "launchers.hpp"
#include "wave_util.hpp"

namespace scrp {

using sc::NodeHdr;

// the most-visited child of a node with children [fc, fc + nc): one packed key per child, visits above, the index inverted below,
// so that the maximum is the LOWEST index among the most visited.  -> the key's winner as (visits, index), wave-uniform
__device__ __forceinline__ void most_visited(const int32_t* N, int fc, int nc, int lane, int* best_n, int* best_i) {
    unsigned long long key = 0;
    for (int i = lane; i < nc; i += 64) {
        const unsigned long long k = (unsigned long long)(uint32_t)N[fc + i] << 32 | (0xffffffffu - (uint32_t)i);
        key = k > key ? k : key;
    }
    key = scw::uniform((uint64_t)scw::wave_max_u64(key));
    *best_n = (int)(uint32_t)(key >> 32);
    *best_i = (int)(0xffffffffu - (uint32_t)key);
}

__global__ __launch_bounds__(64) void k_report(const ReportArgs a) {
    __shared__ int32_t s_n[sc::MAXC];
    const int lane = (int)threadIdx.x;
    const int e = (int)blockIdx.x / a.multipv, r = (int)blockIdx.x - e * a.multipv;
    const int slot = scw::uniform(a.slots ? a.slots[e] : e);
    if (slot < 0 || slot >= a.n_slots) return;   // (the host has checked the list)
    const sc::GameCtl* c = a.ctl + slot;
    const int status = scw::uniform(c->status), ply = scw::uniform(c->ply), sim = scw::uniform(c->sim), n_nodes = scw::uniform(c->n_nodes);
    const size_t nb = (size_t)slot * (size_t)a.node_cap;
    const int32_t* N = a.N + nb;
    const float* W = a.W + nb;
    const uint16_t* MV = a.MV + nb;
    const NodeHdr* H = a.H + nb;

    const bool has_root = n_nodes > 0 && n_nodes <= a.node_cap;
    NodeHdr h0{-1, 0, 0};
    if (has_root) h0 = H[0];
    const int fc0 = scw::uniform(h0.fc), nc0 = scw::uniform((int)h0.nc);
    const bool expanded = has_root && fc0 >= 0 && nc0 > 0 && nc0 <= sc::MAXC && fc0 + nc0 <= n_nodes;
    const bool live = status == sc::ST_ACTIVE && sim > 0 && expanded;
    const int n_lines = live ? (nc0 < a.multipv ? nc0 : a.multipv) : 0;

    if (r == 0) {
        int sum = 0;
        if (expanded)
            for (int i = lane; i < nc0; i += 64) sum += N[fc0 + i];
        sum = scw::wave_sum_i(sum);
        if (lane == 0) {
            SlotInfo o;
            o.status = status;
            o.ply = ply;
            o.sim = sim;
            o.n_nodes = n_nodes;
            o.n_root_children = expanded ? nc0 : 0;
            o.root_children_n = sum;
            o.root_n = has_root ? N[0] : 0;
            o.turn = (status == sc::ST_ACTIVE || status == sc::ST_FINISHED) && ply >= 0 && ply < a.hist_cap
                         ? (int32_t)a.hist[(size_t)slot * (size_t)a.hist_cap + (size_t)ply].turn : -1;
            o.n_lines = n_lines;
            o.pad = 0;
            o.root_w = has_root ? W[0] : 0.f;
            a.info[e] = o;
        }
    }
    if (r >= n_lines) return;

    // the child of rank r
    for (int i = lane; i < nc0; i += 64) s_n[i] = N[fc0 + i];
    scw::wave_sync();
    int mine = -1;
    for (int i = lane; i < nc0; i += 64) {
        const int ni = s_n[i];
        int rank = 0;
        for (int j = 0; j < nc0; j++) {
            const int nj = s_n[j];
            rank += (nj > ni || (nj == ni && j < i)) ? 1 : 0;
        }
        if (rank == r) mine = i;
    }
    const unsigned long long owner = __ballot(mine >= 0);
    if (owner == 0) return;   // (cannot be: the ranks are a permutation of 0 .. nc0 - 1)
    const int child = __builtin_amdgcn_readlane(mine, (int)__builtin_ctzll(owner));

    // the walk
    const size_t row = (size_t)e * (size_t)a.multipv + (size_t)r;
    uint16_t* pv = a.pv + row * (size_t)a.pv_cap;
    int x = fc0 + child, len = 1, end = END_OPEN;
    if (lane == 0 && a.pv_cap > 0) pv[0] = MV[x];
    for (;;) {
        const NodeHdr h = H[x];
        const int fc = scw::uniform(h.fc), nc = scw::uniform((int)h.nc);
        if (fc <= -2) {
            end = fc == -2 ? END_DRAW : fc == -3 ? END_WHITE : END_BLACK;
            break;
        }
        if (fc < 0 || nc <= 0 || nc > sc::MAXC || fc + nc > n_nodes) break;   // unexpanded (or not a node range of this tree)
        int best_n, best_i;
        most_visited(N, fc, nc, lane, &best_n, &best_i);
        if (best_n <= 0) break;   // no visited child
        if (len >= MAX_PV) {
            end = END_DEPTH;
            break;
        }
        x = fc + best_i;
        if (lane == 0 && len < a.pv_cap) pv[len] = MV[x];
        len++;
    }
    if (lane == 0) {
        const int c0 = fc0 + child;
        a.line_child[row] = child;
        a.line_n[row] = N[c0];
        a.line_w[row] = W[c0];
        a.line_prior[row] = a.P[nb + (size_t)c0];
        a.line_len[row] = len;
        a.line_end[row] = end;
    }
}

}  // namespace scrp

namespace scl {
void report(const scrp::ReportArgs& a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(scrp::k_report, dim3((unsigned)a.n * (unsigned)a.multipv), dim3(64), 0, s, a);
}
}  // namespace scl
