// report.hip -- host side of libsc_engine.so: the search report of a self-play handle (sc_selfplay_report,
// sc_selfplay_report_last_timing; include/sc_engine.h).  One kernel launch reads the trees of every requested slot in place
// (report_kernels.hip), one copy brings the packed buffer to the host, and the rows that were written are handed out.
#include <string.h>

#include <chrono>

#include "host_common.hpp"

static_assert(sizeof(scrp::SlotInfo) == sizeof(sc_report_slot) && sizeof(sc_report_slot) == 44, "sc_report_slot layout");
static_assert(offsetof(scrp::SlotInfo, root_w) == offsetof(sc_report_slot, root_w) && offsetof(sc_report_slot, n_lines) == 32,
              "sc_report_slot layout");

namespace {
thread_local float g_kernel_ms = 0.f, g_total_ms = 0.f;

// rows [0, n_lines) of entry i from the packed array to the caller's (which may be null)
template <class T>
void hand_out(T* dst, const std::vector<char>& buf, size_t off, size_t i, size_t multipv, int n_lines) {
    if (dst && n_lines > 0) memcpy(dst + i * multipv, buf.data() + off + i * multipv * sizeof(T), (size_t)n_lines * sizeof(T));
}
}  // namespace

extern "C" {

int sc_selfplay_report(sc_selfplay* sp, int n, const int32_t* slots, int multipv, int pv_cap, sc_report_slot* info, int32_t* line_child,
                       int32_t* line_n, float* line_w, float* line_prior, int32_t* line_len, int32_t* line_end, uint16_t* pv) {
    const auto t_begin = std::chrono::steady_clock::now();
    g_kernel_ms = g_total_ms = 0.f;
    if (!sp || n < 0 || multipv < 1 || multipv > sc::MAXC || pv_cap < 0 || pv_cap > scrp::MAX_PV) return fail("bad argument");
    if (sp->poisoned) return sp_refuse(sp);
    const sc::SpParams& p = sp->p;
    if (n > p.n_slots) return fail("sc_selfplay_report: more entries than slots (a slot may be listed once)");
    if (slots) {
        std::vector<char> seen((size_t)p.n_slots, 0);
        for (int i = 0; i < n; i++) {
            if (slots[i] < 0 || slots[i] >= p.n_slots) return fail("sc_selfplay_report: slot out of range");
            if (seen[(size_t)slots[i]]++) return fail("sc_selfplay_report: slot listed twice");
        }
    }
    // the pending expansion and backup of the last enqueued simulation first: the report sees a fully backed-up tree
    TRY(sp_quiesce(sp, true));
    if (n == 0) return 0;
    const scrp::Packed lay((size_t)n, (size_t)multipv, (size_t)pv_cap);
    TRY(sp->d_report.grow(lay.bytes, [sp] { return hipStreamSynchronize(sp->stream); }));
    for (hipEvent_t& ev : sp->report_ev)
        if (!ev) HIPOK(hipEventCreate(&ev));
    char* d = sp->d_report.p;
    if (slots) HIPOK(hipMemcpyAsync(d + lay.slots, slots, (size_t)n * 4, hipMemcpyHostToDevice, sp->stream));
    scrp::ReportArgs a{};
    a.n = n;
    a.multipv = multipv;
    a.pv_cap = pv_cap;
    a.n_slots = p.n_slots;
    a.node_cap = p.node_cap;
    a.hist_cap = p.hist_cap;
    a.slots = slots ? reinterpret_cast<const int32_t*>(d + lay.slots) : nullptr;
    a.ctl = p.ctl;
    a.hist = p.hist;
    a.N = p.N;
    a.W = p.W;
    a.P = p.P;
    a.MV = p.MV;
    a.H = p.H;
    a.info = reinterpret_cast<scrp::SlotInfo*>(d + lay.info);
    a.line_child = reinterpret_cast<int32_t*>(d + lay.line[0]);
    a.line_n = reinterpret_cast<int32_t*>(d + lay.line[1]);
    a.line_w = reinterpret_cast<float*>(d + lay.line[2]);
    a.line_prior = reinterpret_cast<float*>(d + lay.line[3]);
    a.line_len = reinterpret_cast<int32_t*>(d + lay.line[4]);
    a.line_end = reinterpret_cast<int32_t*>(d + lay.line[5]);
    a.pv = reinterpret_cast<uint16_t*>(d + lay.pv);
    HIPOK(hipEventRecord(sp->report_ev[0], sp->stream));
    scl::report(a, sp->stream);
    HIPOK(hipGetLastError());
    HIPOK(hipEventRecord(sp->report_ev[1], sp->stream));
    std::vector<char> buf(lay.bytes);
    HIPOK(hipMemcpyAsync(buf.data(), d, lay.bytes, hipMemcpyDeviceToHost, sp->stream));
    HIPOK(hipStreamSynchronize(sp->stream));
    HIPOK(hipEventElapsedTime(&g_kernel_ms, sp->report_ev[0], sp->report_ev[1]));

    const scrp::SlotInfo* si = reinterpret_cast<const scrp::SlotInfo*>(buf.data() + lay.info);
    const int32_t* len = reinterpret_cast<const int32_t*>(buf.data() + lay.line[4]);
    const uint16_t* moves = reinterpret_cast<const uint16_t*>(buf.data() + lay.pv);
    const size_t m = (size_t)multipv;
    if (info) memcpy(info, si, (size_t)n * sizeof(sc_report_slot));
    for (size_t i = 0; i < (size_t)n; i++) {
        const int nl = std::min(std::max(si[i].n_lines, 0), multipv);
        hand_out(line_child, buf, lay.line[0], i, m, nl);
        hand_out(line_n, buf, lay.line[1], i, m, nl);
        hand_out(line_w, buf, lay.line[2], i, m, nl);
        hand_out(line_prior, buf, lay.line[3], i, m, nl);
        hand_out(line_len, buf, lay.line[4], i, m, nl);
        hand_out(line_end, buf, lay.line[5], i, m, nl);
        if (!pv) continue;
        for (size_t r = 0; r < (size_t)nl; r++) {   // the moves that were written: min(len, pv_cap) of every line
            const size_t row = i * m + r;
            const size_t k = (size_t)std::min(std::max(len[row], 0), pv_cap);
            if (k) memcpy(pv + row * (size_t)pv_cap, moves + row * (size_t)pv_cap, k * 2);
        }
    }
    g_total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return 0;
}

int sc_selfplay_report_last_timing(float* kernel_ms, float* total_ms) {
    if (kernel_ms) *kernel_ms = g_kernel_ms;
    if (total_ms) *total_ms = g_total_ms;
    return 0;
}

}  // extern "C"
