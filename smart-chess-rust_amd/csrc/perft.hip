// perft.hip -- host side of libsc_engine.so: perft on the device (sc_perft, sc_perft_last_timing; include/sc_engine.h).
//
// The host walks the levels.  Level 0 holds the roots of a chunk of entries; below it a level is counted, scanned and expanded into
// the next level buffer, down to the nodes of depth `depth` - 1, which are counted and summed by root move and never expanded.  After
// each scan the host reads the level's total.  If the children do not fit the next buffer it reads the prefix sums and cuts the
// parents where they cross the capacity, and it finishes each piece, down to the last level, before it expands the next:
// depth-first over breadth-first pieces.  More entries than a buffer holds are chunked the same way.  Every launch and every copy
// is on the null stream.  The workspace -- `depth` level buffers of at most max_frontier records, a count and an offset per record
// of the levels that are expanded, two words per record of the last one -- is allocated for the call (ScopedDev) and freed on
// every path out of it.
#include <chrono>

#include "host_common.hpp"

namespace {

using namespace scpf;
typedef unsigned long long u64;

thread_local float g_kernels_ms = 0.f, g_total_ms = 0.f;

constexpr int DEFAULT_FRONTIER = 1 << 20, MIN_FRONTIER = 256, MAX_FRONTIER = 1 << 24, MAX_DEPTH = 16;

struct Walk {
    int depth = 0;
    bool with_kinds = false;
    ScopedDev<Node> buf[MAX_DEPTH];       // level L: the nodes of depth L of the piece at hand
    uint32_t cap[MAX_DEPTH] = {};
    ScopedDev<uint32_t> cnt[MAX_DEPTH], off[MAX_DEPTH];   // levels that are expanded: off has cap + 1 entries
    ScopedDev<uint32_t> leaf_cnt, leaf_kinds, tile_sum, err;
    std::vector<uint32_t> h_off[MAX_DEPTH];   // the prefix sums of a level that had to be cut
    Totals totals{};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float kernels_ms = 0.f;
    ~Walk() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
    // the launches between two host reads, bracketed (sc_perft_last_timing)
    int begin() {
        HIPOK(hipEventRecord(ev0, nullptr));
        return 0;
    }
    int end() {
        HIPOK(hipGetLastError());
        HIPOK(hipEventRecord(ev1, nullptr));
        HIPOK(hipEventSynchronize(ev1));
        float ms = 0.f;
        HIPOK(hipEventElapsedTime(&ms, ev0, ev1));
        kernels_ms += ms;
        return 0;
    }
    int level(int L, uint32_t m);
};

// the m nodes of depth L in buf[L]: everything below them
int Walk::level(int L, uint32_t m) {
    if (m == 0) return 0;
    if (m > cap[L]) return fail("sc_perft: a level holds more nodes than its buffer");
    if (L == depth - 1) {
        TRY(begin());
        scl::perft_leaf({buf[L].p, 0, m}, {leaf_cnt.p, with_kinds ? leaf_kinds.p : nullptr}, totals, nullptr);
        return end();
    }
    TRY(begin());
    scl::perft_count({buf[L].p, 0, m}, cnt[L].p, nullptr);
    scl::exclusive_scan_u32(m, cnt[L].p, tile_sum.p, off[L].p, off[L].p + m, nullptr);
    TRY(end());
    uint32_t total = 0;
    HIPOK(hipMemcpy(&total, off[L].p + m, 4, hipMemcpyDeviceToHost));
    if (total == 0) return 0;
    const uint32_t room = cap[L + 1];
    const int from_roots = L == 0 ? 1 : 0;
    if (total <= room) {
        TRY(begin());
        scl::perft_expand({{buf[L].p, 0, m}, off[L].p, 0, buf[L + 1].p, room, from_roots, err.p}, nullptr);
        TRY(end());
        return level(L + 1, total);
    }
    std::vector<uint32_t>& h = h_off[L];
    h.resize((size_t)m + 1);
    HIPOK(hipMemcpy(h.data(), off[L].p, ((size_t)m + 1) * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < m; i++)
        if (h[i + 1] < h[i] || h[i + 1] - h[i] > (uint32_t)ROW) return fail("sc_perft: the scan of a level is not one of move counts");
    for (uint32_t p0 = 0; p0 < m;) {
        // the parents [p0, p1) whose children fill the next buffer: the last p1 with off[p1] - off[p0] <= room
        const uint64_t limit = (uint64_t)h[p0] + room;
        const uint32_t p1 = (uint32_t)(std::upper_bound(h.begin() + p0, h.end(), limit, [](uint64_t v, uint32_t x) { return v < x; }) - h.begin()) - 1;
        if (p1 <= p0) return fail("sc_perft: a node has more children than a level buffer holds");
        const uint32_t kids = h[p1] - h[p0];
        if (kids) {
            TRY(begin());
            scl::perft_expand({{buf[L].p, p0, p1 - p0}, off[L].p, h[p0], buf[L + 1].p, room, from_roots, err.p}, nullptr);
            TRY(end());
            TRY(level(L + 1, kids));
        }
        p0 = p1;
    }
    return 0;
}

// min(a * b, limit) without overflow
uint64_t mul_capped(uint64_t a, uint64_t b, uint64_t limit) { return a && b > limit / a ? limit : std::min(a * b, limit); }

}  // namespace

extern "C" {

int sc_perft(int device_id, int n, const sc_positions* bases, const int32_t* base_idx, const uint16_t* moves, const uint32_t* move_off, int depth,
             int max_frontier, uint64_t* nodes, uint64_t* kinds, uint16_t* div_moves, uint64_t* div_nodes, int32_t* n_div, int32_t* status) {
    const auto t_begin = std::chrono::steady_clock::now();
    g_kernels_ms = g_total_ms = 0.f;
    if (n < 0 || n > MAX_ENTRIES) return fail("sc_perft: n outside 0..2^24-1");
    if (depth < 0 || depth > MAX_DEPTH) return fail("sc_perft: depth outside 0..16");
    if (max_frontier != 0 && (max_frontier < MIN_FRONTIER || max_frontier > MAX_FRONTIER)) return fail("sc_perft: max_frontier is 0 or in 256..2^24");
    if (!nodes) return fail("sc_perft: nodes is required");
    if ((div_moves == nullptr) != (div_nodes == nullptr)) return fail("sc_perft: div_moves and div_nodes go together");
    if (moves && !move_off) return fail("sc_perft: moves without move_off");
    if (n == 0) return 0;
    if (move_off) {
        TRY(check_traces(n, move_off, nullptr));
        if (move_off[n] != move_off[0] && !moves) return fail("sc_perft: move_off without moves");
    }
    TRY(use_device(nullptr, device_id));
    const sc::Position* d_bases = nullptr;
    TRY(positions_bases(bases, base_idx, n, device_id, false, "sc_perft", &d_bases));

    const size_t N = (size_t)n;
    const uint32_t frontier = (uint32_t)(max_frontier ? max_frontier : DEFAULT_FRONTIER);
    const bool want_div = div_moves != nullptr;
    Walk w;
    w.depth = depth;
    w.with_kinds = kinds != nullptr && depth >= 1;
    ScopedDev<uint16_t> d_moves, d_div_moves;
    ScopedDev<uint32_t> d_off;
    ScopedDev<int32_t> d_bidx, d_status, d_n_div;
    ScopedDev<u64> d_nodes, d_kinds, d_div_nodes;
    const uint32_t m_first = move_off ? move_off[0] : 0, m_total = move_off ? move_off[n] : 0;
    if (move_off) {
        HIPOK(d_moves.alloc(m_total));
        HIPOK(d_off.alloc(N + 1));
        if (m_total > m_first) HIPOK(hipMemcpy(d_moves.p + m_first, moves + m_first, (size_t)(m_total - m_first) * 2, hipMemcpyHostToDevice));
        HIPOK(hipMemcpy(d_off.p, move_off, (N + 1) * 4, hipMemcpyHostToDevice));
    }
    if (d_bases) {
        HIPOK(d_bidx.alloc(N));
        HIPOK(hipMemcpy(d_bidx.p, base_idx, N * 4, hipMemcpyHostToDevice));
    }
    HIPOK(d_status.alloc(N));
    HIPOK(w.err.alloc(1));
    HIPOK(hipMemset(w.err.p, 0, 4));
    HIPOK(d_nodes.alloc(N));
    HIPOK(hipMemset(d_nodes.p, 0, N * 8));
    if (w.with_kinds) {
        HIPOK(d_kinds.alloc(N * KINDS));
        HIPOK(hipMemset(d_kinds.p, 0, N * KINDS * 8));
    }
    if (depth >= 1 && (n_div || want_div)) HIPOK(d_n_div.alloc(N));
    if (depth >= 1 && want_div) {
        HIPOK(d_div_moves.alloc(N * ROW));
        HIPOK(d_div_nodes.alloc(N * ROW));
        HIPOK(hipMemset(d_div_nodes.p, 0, N * ROW * 8));
    }
    // level L never holds more than 218^L nodes per entry of a chunk
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(N, frontier);
    uint64_t bound = chunk;
    for (int L = 0; L < depth; L++) {
        w.cap[L] = (uint32_t)std::min<uint64_t>(bound, frontier);
        if (L > 0 && w.cap[L] < (uint32_t)ROW) w.cap[L] = (uint32_t)ROW;   // a level buffer holds the children of one node
        HIPOK(w.buf[L].alloc(w.cap[L]));
        if (L < depth - 1) {
            HIPOK(w.cnt[L].alloc(w.cap[L]));
            HIPOK(w.off[L].alloc((size_t)w.cap[L] + 1));
        }
        bound = mul_capped(bound, 218, frontier);
    }
    if (depth >= 1) {
        const uint32_t widest = *std::max_element(w.cap, w.cap + depth);
        HIPOK(w.leaf_cnt.alloc(w.cap[depth - 1]));
        if (w.with_kinds) HIPOK(w.leaf_kinds.alloc(2 * (size_t)w.cap[depth - 1]));
        HIPOK(w.tile_sum.alloc(widest / scl::SCAN_TILE + 1));
    }
    HIPOK(hipEventCreate(&w.ev0));
    HIPOK(hipEventCreate(&w.ev1));
    w.totals = {n, d_nodes.p, w.with_kinds ? d_kinds.p : nullptr, d_div_nodes.p, w.err.p};

    for (size_t e0 = 0; e0 < N; e0 += chunk) {
        const int cn = (int)std::min<size_t>(chunk, N - e0);
        TRY(w.begin());
        scl::perft_roots({(int)e0, cn, d_moves.p, d_off.p, {d_bases, d_bidx.p}, depth >= 1 ? w.buf[0].p : nullptr, depth >= 1 ? w.cap[0] : 0u,
                          d_status.p, d_n_div.p, d_div_moves.p, w.err.p},
                         nullptr);
        TRY(w.end());
        if (depth >= 1) TRY(w.level(0, (uint32_t)cn));
    }
    if (depth == 1 && want_div) {
        TRY(w.begin());
        scl::perft_div_ones(n, d_n_div.p, d_div_nodes.p, nullptr);
        TRY(w.end());
    }
    uint32_t err = 0;
    HIPOK(hipMemcpy(&err, w.err.p, 4, hipMemcpyDeviceToHost));
    if (err) return fail("sc_perft: a kernel found a count that does not match its scan, or an index past its buffer (flags " + std::to_string(err) + "); nothing was written");

    std::vector<int32_t> h_status(N);
    HIPOK(hipMemcpy(h_status.data(), d_status.p, N * 4, hipMemcpyDeviceToHost));
    if (depth == 0) {
        for (size_t i = 0; i < N; i++) nodes[i] = h_status[i] == 0 ? 1 : 0;
        if (kinds)
            for (size_t i = 0; i < N; i++)
                for (int k = 0; k < KINDS; k++) kinds[i * KINDS + k] = k == 0 ? nodes[i] : 0;
        if (want_div) {
            std::fill(div_moves, div_moves + N * ROW, (uint16_t)0);
            std::fill(div_nodes, div_nodes + N * ROW, (uint64_t)0);
        }
        if (n_div) std::fill(n_div, n_div + N, 0);
    } else {
        HIPOK(hipMemcpy(nodes, d_nodes.p, N * 8, hipMemcpyDeviceToHost));
        if (kinds) {
            HIPOK(hipMemcpy(kinds, d_kinds.p, N * KINDS * 8, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < N; i++) kinds[i * KINDS] = nodes[i];
        }
        if (want_div) {
            HIPOK(hipMemcpy(div_moves, d_div_moves.p, N * ROW * 2, hipMemcpyDeviceToHost));
            HIPOK(hipMemcpy(div_nodes, d_div_nodes.p, N * ROW * 8, hipMemcpyDeviceToHost));
        }
        if (n_div) HIPOK(hipMemcpy(n_div, d_n_div.p, N * 4, hipMemcpyDeviceToHost));
    }
    if (status) std::copy(h_status.begin(), h_status.end(), status);
    g_kernels_ms = w.kernels_ms;
    g_total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return 0;
}

int sc_perft_last_timing(float* kernels_ms, float* total_ms) {
    if (kernels_ms) *kernels_ms = g_kernels_ms;
    if (total_ms) *total_ms = g_total_ms;
    return 0;
}

}  // extern "C"
