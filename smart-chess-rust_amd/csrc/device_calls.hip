// device_calls.hip -- host side of libsc_engine.so: the calls on device tensors (forward, losses, agreement, minibatches, merged positions).
//
// sc_forward_device / sc_score_positions / sc_compare_engines (include/sc_engine.h).  The positions are cut into slices of
// SCORE_SLICE (the figure sc_encode_steps uses), so the scratch of a call is bounded whatever its size: enqueue_forward's own
// 256 MB of value-head features and 256 MB of split-K partials (d_hval / d_vpart, the buffers sc_forward_batch uses: one set per
// engine) and -- scoring only -- 153 MB of log-probability rows, which the scoring
// kernels read back while the slice is still in the Infinity Cache.  A position is one workgroup of the tower, one row of
// value_fc1's tiles and one wavefront of the scoring kernels: its results do not depend on the slice it falls in.
#include "host_common.hpp"

namespace {
constexpr int SCORE_SLICE = 8192;

// Work of these calls runs on the CALLER's stream.  begin: the stream waits for the engine's earlier work (host-pointer calls,
// self-play steps, earlier device calls -- the engine's stream waits for each of those in end).  The scratch is therefore
// never used by two calls at once, and growing it waits on the host for the engine's stream only.
struct DevCall {
    sc_engine* e;
    hipStream_t st;
    bool armed = false;
    int begin() {
        if (!e->dv_ev) HIPOK(hipEventCreateWithFlags(&e->dv_ev, hipEventDisableTiming));
        if (st != e->stream) {
            HIPOK(hipEventRecord(e->dv_ev, e->stream));
            HIPOK(hipStreamWaitEvent(st, e->dv_ev, 0));
        }
        armed = true;
        return 0;
    }
    ~DevCall() {   // on every path out of the call: later work of the engine waits for what was enqueued
        if (armed && st != e->stream && hipEventRecord(e->dv_ev, st) == hipSuccess) (void)hipStreamWaitEvent(e->stream, e->dv_ev, 0);
    }
};
}  // namespace

static int dev_slice_cap(int n) {
    int c = 64;
    while (c < n && c < SCORE_SLICE) c *= 2;
    return c;
}
static int dev_reserve(sc_engine* e, int n, bool want_logp, size_t pp_floats) {
    const size_t cap = (size_t)dev_slice_cap(n);
    TRY(engine_reserve_hv(e, (int)cap));
    TRY(engine_grow(e, e->dv_value, cap));
    if (want_logp) TRY(engine_grow(e, e->dv_logp, cap * 4672));
    if (pp_floats) TRY(engine_grow(e, e->dv_pp, std::max<size_t>(pp_floats, 4 * SCORE_SLICE)));
    return 0;
}

// tower + value head of one slice on device tensors (reference layout: meta rows of 7): sc_forward_batch's three launches
static void dev_forward_slice(sc_engine* e, int n, const int8_t* boards, const int32_t* meta, float* logp, float* value, hipStream_t st) {
    enqueue_forward(e, n, boards, meta, 7, nullptr, nullptr, nullptr, value, logp, nullptr, -1, st);
}

static int check_row_alignment(std::initializer_list<std::pair<const void*, const char*>> ptrs) {
    for (const auto& x : ptrs)
        if (reinterpret_cast<uintptr_t>(x.first) & 15) return fail(std::string(x.second) + ": rows are read 16 bytes at a time, the pointer must be 16-byte aligned");
    return 0;
}

extern "C" {

int sc_forward_device(sc_engine* e, int n, const int8_t* boards, const int32_t* meta, void* stream, float* logp, float* value) {
    if (!e || !boards || !meta || !value || n < 0) return fail("bad argument");
    TRY(use_device(e, 0));
    TRY(check_device_ptrs({{boards, "boards"}, {meta, "meta"}, {logp, "logp"}, {value, "value"}}, e->device));
    if (n == 0) return 0;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    TRY(dev_reserve(e, n, false, 0));
    DevCall call{e, st};
    TRY(call.begin());
    for (int p0 = 0; p0 < n; p0 += SCORE_SLICE) {
        const int m = std::min(SCORE_SLICE, n - p0);
        dev_forward_slice(e, m, boards + (size_t)p0 * 7168, meta + (size_t)p0 * 7, logp ? logp + (size_t)p0 * 4672 : nullptr, value + p0, st);
    }
    HIPOK(hipGetLastError());
    return 0;
}

int sc_score_positions(sc_engine* e, int n, const int8_t* boards, const int32_t* meta, const float* dist, const float* dist_legal,
                       const uint16_t* legal_idx, const int32_t* n_legal, const float* outcome, void* stream, float* ce, float* se,
                       float* ent, float* value, double* summary) {
    if (!e || !boards || !meta || !outcome || n < 0) return fail("bad argument");
    const bool sparse = dist_legal || legal_idx || n_legal;
    if (dist && sparse) return fail("give the visit shares in ONE form: dist, or dist_legal + legal_idx + n_legal");
    if (!dist && !(dist_legal && legal_idx && n_legal)) return fail("the visit shares are missing: dist, or dist_legal + legal_idx + n_legal");
    TRY(use_device(e, 0));
    TRY(check_device_ptrs({{boards, "boards"}, {meta, "meta"}, {dist, "dist"}, {dist_legal, "dist_legal"}, {legal_idx, "legal_idx"},
                           {n_legal, "n_legal"}, {outcome, "outcome"}, {ce, "ce"}, {se, "se"}, {ent, "ent"}, {value, "value"},
                           {summary, "summary"}}, e->device));
    TRY(check_row_alignment({{dist, "dist"}}));
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) {
        if (summary) HIPOK(hipMemsetAsync(summary, 0, 5 * sizeof(double), st));
        return 0;
    }
    TRY(dev_reserve(e, n, true, (size_t)3 * n));
    DevCall call{e, st};
    TRY(call.begin());
    float* w_ce = ce ? ce : e->dv_pp.p;
    float* w_se = se ? se : e->dv_pp.p + (size_t)n;
    float* w_ent = ent ? ent : e->dv_pp.p + (size_t)2 * n;
    for (int p0 = 0; p0 < n; p0 += SCORE_SLICE) {
        const int m = std::min(SCORE_SLICE, n - p0);
        dev_forward_slice(e, m, boards + (size_t)p0 * 7168, meta + (size_t)p0 * 7, e->dv_logp.p, e->dv_value.p, st);
        scsc::ScoreArgs a{};
        a.n = m;
        a.logp = e->dv_logp.p;
        a.value = e->dv_value.p;
        a.dist = dist ? dist + (size_t)p0 * 4672 : nullptr;
        a.dist_legal = dist ? nullptr : dist_legal + (size_t)p0 * 224;
        a.legal_idx = dist ? nullptr : legal_idx + (size_t)p0 * 224;
        a.n_legal = dist ? nullptr : n_legal + p0;
        a.outcome = outcome + p0;
        a.ce = w_ce + p0;
        a.se = w_se + p0;
        a.ent = w_ent + p0;
        a.value_out = value ? value + p0 : nullptr;
        scl::score_positions(a, st);
    }
    if (summary) {
        scsc::SummaryArgs s{};
        s.n = n;
        s.mode = 0;
        s.x0 = w_ce;
        s.x1 = w_se;
        s.x2 = w_ent;
        s.out = summary;
        scl::score_summary(s, st);
    }
    HIPOK(hipGetLastError());
    return 0;
}

int sc_compare_engines(sc_engine* ea, sc_engine* eb, int n, const int8_t* boards, const int32_t* meta, void* stream, float* tv,
                       float* dv, double* summary) {
    if (!ea || !eb || !boards || !meta || n < 0) return fail("bad argument");
    TRY(use_device(ea, 0));
    if (ea->device != eb->device)
        return fail("the two engines are on devices " + std::to_string(ea->device) + " and " + std::to_string(eb->device) +
                    ": sc_compare_engines needs both on the GPU that holds the positions");
    TRY(check_device_ptrs({{boards, "boards"}, {meta, "meta"}, {tv, "tv"}, {dv, "dv"}, {summary, "summary"}}, ea->device));
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) {
        if (summary) HIPOK(hipMemsetAsync(summary, 0, 9 * sizeof(double), st));
        return 0;
    }
    const bool same = ea == eb;   // one engine against itself: one forward pass, its rows on both sides
    TRY(dev_reserve(ea, n, true, (size_t)2 * n));
    if (!same) TRY(dev_reserve(eb, n, true, 0));
    DevCall call_a{ea, st}, call_b{eb, st};
    TRY(call_a.begin());
    if (!same) TRY(call_b.begin());
    float* w_tv = tv ? tv : ea->dv_pp.p;
    float* w_dv = dv ? dv : ea->dv_pp.p + (size_t)n;
    for (int p0 = 0; p0 < n; p0 += SCORE_SLICE) {
        const int m = std::min(SCORE_SLICE, n - p0);
        dev_forward_slice(ea, m, boards + (size_t)p0 * 7168, meta + (size_t)p0 * 7, ea->dv_logp.p, ea->dv_value.p, st);
        if (!same) dev_forward_slice(eb, m, boards + (size_t)p0 * 7168, meta + (size_t)p0 * 7, eb->dv_logp.p, eb->dv_value.p, st);
        scsc::CompareArgs a{};
        a.n = m;
        a.logp1 = ea->dv_logp.p;
        a.logp2 = eb->dv_logp.p;
        a.value1 = ea->dv_value.p;
        a.value2 = eb->dv_value.p;
        a.tv = w_tv + p0;
        a.dv = w_dv + p0;
        scl::compare_rows(a, st);
    }
    if (summary) {
        scsc::SummaryArgs s{};
        s.n = n;
        s.mode = 1;
        s.x0 = w_tv;
        s.x1 = w_dv;
        s.x2 = nullptr;
        s.out = summary;
        scl::score_summary(s, st);
    }
    HIPOK(hipGetLastError());
    return 0;
}

// Rows of the compact training tensors, chosen by index, as a trainer-layout minibatch (include/sc_engine.h): one launch of
// k_gather_batch behind the zeroing of n_bad, on the caller's stream.  No engine, no scratch, nothing kept after the call.
int sc_gather_batch(int device_id, int n_src, int n_batch, const int32_t* rows, const uint8_t* mirror, const int8_t* boards,
                    const int32_t* meta, const float* dist_legal, const uint16_t* legal_idx, const int32_t* n_legal,
                    const float* outcome, void* stream, float* out_boards, float* out_meta, float* out_dist, float* out_outcome,
                    int32_t* n_bad) {
    if (n_src < 0 || n_batch < 0 || !rows || !boards || !meta || !dist_legal || !legal_idx || !n_legal || !outcome) return fail("bad argument");
    TRY(use_device(nullptr, device_id));
    TRY(check_device_ptrs({{rows, "rows"}, {mirror, "mirror"}, {boards, "boards"}, {meta, "meta"}, {dist_legal, "dist_legal"},
                           {legal_idx, "legal_idx"}, {n_legal, "n_legal"}, {outcome, "outcome"}, {out_boards, "out_boards"},
                           {out_meta, "out_meta"}, {out_dist, "out_dist"}, {out_outcome, "out_outcome"}, {n_bad, "n_bad"}}, device_id));
    TRY(check_row_alignment({{boards, "boards"}, {dist_legal, "dist_legal"}, {legal_idx, "legal_idx"}, {out_boards, "out_boards"},
                             {out_dist, "out_dist"}}));
    if (n_batch == 0) return 0;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_bad) HIPOK(hipMemsetAsync(n_bad, 0, sizeof(int32_t), st));
    scbt::GatherArgs a{};
    a.n_src = n_src;
    a.n_batch = n_batch;
    a.rows = rows;
    a.mirror = mirror;
    a.boards = boards;
    a.meta = meta;
    a.dist_legal = dist_legal;
    a.legal_idx = legal_idx;
    a.n_legal = n_legal;
    a.outcome = outcome;
    a.out_boards = out_boards;
    a.out_meta = out_meta;
    a.out_dist = out_dist;
    a.out_outcome = out_outcome;
    a.n_bad = n_bad;
    scl::gather_batch(a, st);
    HIPOK(hipGetLastError());
    return 0;
}

// Identical rows of the compact training tensors merged into one row each (include/sc_engine.h): the kernels of
// merge_kernels.hip on the caller's stream, their scratch in the caller's workspace.  No engine, no host wait, nothing kept.
int sc_merge_positions_workspace(int n_in, size_t* bytes) {
    if (n_in < 0 || n_in > scmg::MAX_IN || !bytes) return fail("bad argument");
    *bytes = scmg::workspace(n_in).bytes;
    return 0;
}

int sc_merge_positions(int device_id, int n_src, int n_in, const int32_t* rows, const int8_t* boards, const int32_t* meta,
                       const float* dist_legal, const uint16_t* legal_idx, const int32_t* n_legal, const float* outcome, int key_bits,
                       void* workspace, size_t workspace_bytes, void* stream, int8_t* out_boards, int32_t* out_meta, float* out_dist_legal,
                       uint16_t* out_legal_idx, int32_t* out_n_legal, float* out_outcome, int32_t* out_count, int32_t* out_first,
                       int32_t* group_of, int32_t* counts) {
    if (n_src < 0 || n_in < 0 || n_in > scmg::MAX_IN || key_bits < 0 || key_bits > 128 || !boards || !meta || !dist_legal || !legal_idx ||
        !n_legal || !outcome)
        return fail("bad argument");
    if (!rows && n_in > n_src) return fail("bad argument: without rows, position p is row p and n_in may not exceed n_src");
    const scmg::Workspace L = scmg::workspace(n_in);
    if (n_in > 0 && (!workspace || workspace_bytes < L.bytes))
        return fail("workspace: " + std::to_string(L.bytes) + " bytes are needed (sc_merge_positions_workspace)");
    TRY(use_device(nullptr, device_id));
    TRY(check_device_ptrs({{rows, "rows"}, {boards, "boards"}, {meta, "meta"}, {dist_legal, "dist_legal"}, {legal_idx, "legal_idx"},
                           {n_legal, "n_legal"}, {outcome, "outcome"}, {workspace, "workspace"}, {out_boards, "out_boards"},
                           {out_meta, "out_meta"}, {out_dist_legal, "out_dist_legal"}, {out_legal_idx, "out_legal_idx"},
                           {out_n_legal, "out_n_legal"}, {out_outcome, "out_outcome"}, {out_count, "out_count"},
                           {out_first, "out_first"}, {group_of, "group_of"}, {counts, "counts"}}, device_id));
    TRY(check_row_alignment({{boards, "boards"}, {legal_idx, "legal_idx"}, {out_boards, "out_boards"}, {out_legal_idx, "out_legal_idx"}}));
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (counts) HIPOK(hipMemsetAsync(counts, 0, 4 * sizeof(int32_t), st));
    if (n_in == 0) return 0;
    scmg::MergeArgs a{};
    a.n_src = n_src;
    a.n_in = n_in;
    a.key_bits = key_bits;
    a.rows = rows;
    a.boards = boards;
    a.meta = meta;
    a.dist_legal = dist_legal;
    a.legal_idx = legal_idx;
    a.n_legal = n_legal;
    a.outcome = outcome;
    a.ws = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    a.out_boards = out_boards;
    a.out_meta = out_meta;
    a.out_dist_legal = out_dist_legal;
    a.out_legal_idx = out_legal_idx;
    a.out_n_legal = out_n_legal;
    a.out_outcome = out_outcome;
    a.out_count = out_count;
    a.out_first = out_first;
    a.group_of = group_of;
    a.counts = counts;
    const char* why = nullptr;
    const hipError_t err = scl::merge_positions(a, st, &why);
    if (why) return fail(why);
    HIPOK(err);
    return 0;
}

}  // extern "C"
