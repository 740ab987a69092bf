// traces.hip -- host side of libsc_engine.so: trace files read on the device (sc_traces_*; include/sc_engine.h).  The bytes of the
// files go up in one copy; trace_kernels.hip counts and checks them, the one scan (scan_kernels.hip) turns the counts into bases,
// one small copy brings the per-file results to the host, which sizes the set's arrays, and the second pass fills them.  The set
// keeps the packed arrays on the device, where sc_traces_encode_device (encode_steps.hip) reads them, and a host copy of what is
// per file, so that its accessors need no device work but the copies sc_traces_get is asked for.
#include <string.h>

#include "host_common.hpp"

static thread_local float g_traces_ms[2] = {0.f, 0.f};   // last sc_traces_read of this thread: the two passes (HIP events)

const uint32_t* traces_range_off(const sc_traces* t, int g0) {
    const uint32_t p0 = t->move_off[(size_t)g0];
    if (p0 == 0) return t->move_off.data() + g0;
    std::lock_guard<std::mutex> lk(t->mu);
    std::vector<uint32_t>& v = t->range_off[g0];
    if (v.empty()) {
        v.assign(t->move_off.begin() + g0, t->move_off.end());
        for (uint32_t& x : v) x -= p0;
    }
    return v.data();
}

namespace {
struct Events {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // around the first pass with its scans, around the second
    ~Events() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};
template <class T>
int to_host(std::vector<T>& v, const T* d, size_t n) {
    v.resize(n);
    if (n) HIPOK(hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}
std::vector<uint32_t> prefix(const std::vector<uint32_t>& cnt, uint64_t* total) {
    std::vector<uint32_t> off(cnt.size() + 1, 0);
    uint64_t sum = 0;
    for (size_t i = 0; i < cnt.size(); i++) {
        sum += cnt[i];
        off[i + 1] = (uint32_t)sum;
    }
    *total = sum;
    return off;
}
}  // namespace

extern "C" {

int sc_traces_read(int device_id, int n, const char* text, const uint64_t* text_off, sc_traces** out) {
    if (out) *out = nullptr;
    if (n < 0 || !out || (n > 0 && !text_off)) return fail("bad argument");
    for (int g = 0; g < n; g++)
        if (text_off[g + 1] < text_off[g]) return fail("sc_traces_read: text_off is not monotonic (file " + std::to_string(g) + ")");
    if (n > 0 && text_off[n] >= ((uint64_t)1 << 32)) return fail("sc_traces_read: 4 GiB of text or more in one call (text_off[n] must be below 2^32)");
    if (n > 0 && text_off[n] > text_off[0] && !text) return fail("bad argument");
    TRY(use_device(nullptr, device_id));
    sc_traces* t = new sc_traces();
    struct Guard {
        sc_traces* p;
        ~Guard() { sc_traces_destroy(p); }
    } guard{t};
    t->device = device_id;
    t->n = n;
    t->move_off.assign(1, 0);
    t->child_base.assign(1, 0);
    t->open_off.assign(1, 0);
    g_traces_ms[0] = g_traces_ms[1] = 0.f;
    if (n > 0) {
        const size_t N = (size_t)n, bytes = (size_t)(text_off[n] - text_off[0]);
        std::vector<uint64_t> off(text_off, text_off + n + 1);
        for (uint64_t& x : off) x -= text_off[0];
        // the call's device memory: the text (16 readable bytes behind it: the kernels load on the buffer's 16-byte grid) and
        // what is per file
        ScopedDev<char> d_text, d_tmp;
        uint64_t* d_off;
        uint32_t *d_base[3], *d_tile, *d_total;
        sctr::Files F{};
        ArenaLayout L;
        L.add(&d_off, N + 1);
        L.add(&F.status, N);
        L.add(&F.err_at, N);
        L.add(&F.n_steps, N);
        L.add(&F.n_children, N);
        L.add(&F.n_opening, N);
        L.add(&F.outcome, N * 3);
        L.add(&F.has_fen, N);
        L.add(&F.fen, N * sctr::FEN_CAP);
        for (uint32_t*& b : d_base) L.add(&b, N);
        L.add(&d_tile, (N + scl::SCAN_TILE - 1) / scl::SCAN_TILE);
        L.add(&d_total, 3);
        HIPOK(d_text.alloc(bytes + 16));
        HIPOK(d_tmp.alloc(L.bytes));
        L.bind(d_tmp.p);
        Events E;
        for (hipEvent_t& e : E.ev) HIPOK(hipEventCreate(&e));
        if (bytes) HIPOK(hipMemcpy(d_text.p, text + text_off[0], bytes, hipMemcpyHostToDevice));
        HIPOK(hipMemset(d_text.p + bytes, ' ', 16));
        HIPOK(hipMemcpy(d_off, off.data(), (N + 1) * 8, hipMemcpyHostToDevice));
        const sctr::Text T{n, d_text.p, d_off};
        HIPOK(hipEventRecord(E.ev[0], nullptr));
        scl::trace_count(T, F, nullptr);
        scl::exclusive_scan_u32((uint32_t)n, F.n_steps, d_tile, d_base[0], d_total + 0, nullptr);
        scl::exclusive_scan_u32((uint32_t)n, F.n_children, d_tile, d_base[1], d_total + 1, nullptr);
        scl::exclusive_scan_u32((uint32_t)n, F.n_opening, d_tile, d_base[2], d_total + 2, nullptr);
        HIPOK(hipEventRecord(E.ev[1], nullptr));
        HIPOK(hipGetLastError());
        // the per-file results: the host sizes the set's arrays from them (this copy waits for the first pass)
        TRY(to_host(t->status, F.status, N));
        TRY(to_host(t->err_at, F.err_at, N));
        TRY(to_host(t->n_steps, F.n_steps, N));
        TRY(to_host(t->n_children, F.n_children, N));
        TRY(to_host(t->n_opening, F.n_opening, N));
        TRY(to_host(t->outcome, F.outcome, N * 3));
        TRY(to_host(t->has_fen, F.has_fen, N));
        TRY(to_host(t->fen, F.fen, N * sctr::FEN_CAP));
        uint64_t P = 0, C = 0, O = 0;
        t->move_off = prefix(t->n_steps, &P);
        t->child_base = prefix(t->n_children, &C);
        t->open_off = prefix(t->n_opening, &O);
        if (P >> 32 || C >> 32 || O >> 32) return fail("sc_traces_read: more than 2^32 plies or children in one call");
        std::vector<int32_t> over(N);
        for (size_t g = 0; g < N; g++)
            over[g] = t->status[g] < 0 ? 300000 - t->status[g] : (t->n_opening[g] || t->has_fen[g]) ? 400000 : 0;
        HIPOK(dalloc(&t->d_moves, (size_t)P));
        HIPOK(dalloc(&t->d_child_off, (size_t)P + 1));
        HIPOK(dalloc(&t->d_child_mv, (size_t)C));
        HIPOK(dalloc(&t->d_child_n, (size_t)C));
        HIPOK(dalloc(&t->d_opening, (size_t)O));
        HIPOK(dalloc(&t->d_over, N));
        HIPOK(hipMemcpy(t->d_over, over.data(), N * 4, hipMemcpyHostToDevice));
        const uint32_t c_total = (uint32_t)C;
        HIPOK(hipMemcpy(t->d_child_off + P, &c_total, 4, hipMemcpyHostToDevice));
        const sctr::Packed K{d_base[0], d_base[1], d_base[2], t->d_moves, t->d_child_off, t->d_child_mv, t->d_child_n, t->d_opening};
        HIPOK(hipEventRecord(E.ev[2], nullptr));
        scl::trace_emit(T, F, K, nullptr);
        HIPOK(hipEventRecord(E.ev[3], nullptr));
        HIPOK(hipGetLastError());
        HIPOK(hipDeviceSynchronize());
        HIPOK(hipEventElapsedTime(&g_traces_ms[0], E.ev[0], E.ev[1]));
        HIPOK(hipEventElapsedTime(&g_traces_ms[1], E.ev[2], E.ev[3]));
    }
    guard.p = nullptr;
    *out = t;
    return 0;
}

void sc_traces_destroy(sc_traces* t) {
    if (!t) return;
    if (hipSetDevice(t->device) == hipSuccess) dfree({t->d_moves, t->d_child_off, t->d_child_mv, t->d_child_n, t->d_opening, t->d_over});
    delete t;
}

int sc_traces_count(const sc_traces* t) { return t ? t->n : fail("null handle"); }

int sc_traces_summary(const sc_traces* t, int32_t* status, uint32_t* err_at, uint32_t* n_steps, uint32_t* n_children, uint32_t* n_opening,
                      int32_t* outcome, int32_t* has_fen) {
    if (!t) return fail("null handle");
    if (status) std::copy(t->status.begin(), t->status.end(), status);
    if (err_at) std::copy(t->err_at.begin(), t->err_at.end(), err_at);
    if (n_steps) std::copy(t->n_steps.begin(), t->n_steps.end(), n_steps);
    if (n_children) std::copy(t->n_children.begin(), t->n_children.end(), n_children);
    if (n_opening) std::copy(t->n_opening.begin(), t->n_opening.end(), n_opening);
    if (outcome) std::copy(t->outcome.begin(), t->outcome.end(), outcome);
    if (has_fen) std::copy(t->has_fen.begin(), t->has_fen.end(), has_fen);
    return 0;
}

int sc_traces_get(const sc_traces* t, int g0, int n, uint32_t* move_off, uint16_t* moves, uint32_t* child_off, uint16_t* child_mv,
                  uint32_t* child_n, uint32_t* open_off, uint16_t* opening) {
    if (!t || g0 < 0 || n < 0 || (int64_t)g0 + n > t->n) return fail("bad argument");
    const size_t a = (size_t)g0, b = a + (size_t)n;
    const uint32_t p0 = t->move_off[a], p1 = t->move_off[b], c0 = t->child_base[a], c1 = t->child_base[b], q0 = t->open_off[a], q1 = t->open_off[b];
    for (size_t g = a; g <= b; g++) {
        if (move_off) move_off[g - a] = t->move_off[g] - p0;
        if (open_off) open_off[g - a] = t->open_off[g] - q0;
    }
    if (!(moves || child_off || child_mv || child_n || opening)) return 0;
    TRY(use_device(nullptr, t->device));
    if (moves && p1 > p0) HIPOK(hipMemcpy(moves, t->d_moves + p0, (size_t)(p1 - p0) * 2, hipMemcpyDeviceToHost));
    if (child_off) {
        if (t->n == 0) child_off[0] = 0;
        else HIPOK(hipMemcpy(child_off, t->d_child_off + p0, ((size_t)(p1 - p0) + 1) * 4, hipMemcpyDeviceToHost));
        for (uint32_t p = 0; p <= p1 - p0; p++) child_off[p] -= c0;
    }
    if (child_mv && c1 > c0) HIPOK(hipMemcpy(child_mv, t->d_child_mv + c0, (size_t)(c1 - c0) * 2, hipMemcpyDeviceToHost));
    if (child_n && c1 > c0) HIPOK(hipMemcpy(child_n, t->d_child_n + c0, (size_t)(c1 - c0) * 4, hipMemcpyDeviceToHost));
    if (opening && q1 > q0) HIPOK(hipMemcpy(opening, t->d_opening + q0, (size_t)(q1 - q0) * 2, hipMemcpyDeviceToHost));
    return 0;
}

int sc_traces_fen(const sc_traces* t, int g, char* buf, int cap) {
    if (!t || g < 0 || g >= t->n || cap < 0 || (cap > 0 && !buf)) return fail("bad argument");
    if (!t->has_fen[(size_t)g]) {
        if (cap > 0) buf[0] = 0;
        return 0;
    }
    return copy_text(std::string(t->fen.data() + (size_t)g * sctr::FEN_CAP), buf, cap);
}

int sc_traces_last_timing(float* count_ms, float* emit_ms) {
    if (count_ms) *count_ms = g_traces_ms[0];
    if (emit_ms) *emit_ms = g_traces_ms[1];
    return 0;
}

}  // extern "C"
