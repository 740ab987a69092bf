// trace_write.hip -- host side of libsc_engine.so: trace files written on the device (sc_traces_format, sc_selfplay_traces_json,
// sc_selfplay_write_traces_json; include/sc_engine.h).  The host builds what is per game -- the frames: the text in front of the
// steps and behind them, taken from the host writer itself -- and one word per ply that says where the ply is read; the kernels
// (trace_write_kernels.hip) count the bytes of every ply, the one scan (scan_kernels.hip) places heads, plies and tails, the
// second pass writes the text, one copy brings it to the host.  The host writer (trace_json.hpp) stays the yardstick: the bytes
// are its bytes.
#include <stdio.h>
#include <string.h>

#include "host_common.hpp"
#include "trace_fmt.hpp"
#include "trace_json.hpp"

static thread_local float g_fmt_ms[2] = {0.f, 0.f};   // last format call of this thread: the two passes (HIP events)

void TraceWriter::release() {
    if (stream) (void)hipStreamSynchronize(stream);
    arena.release();
    text.release();
    if (pinned) (void)hipHostFree(pinned);
    pinned = nullptr;
    pinned_cap = 0;
    for (hipEvent_t& e : ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    if (stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
}

namespace {

constexpr uint64_t GROUP_LIMIT = (uint64_t)1 << 31;   // bytes of text one emitting pass writes (its offsets are uint32)

// the packed arrays of a call on the host (sc_traces_format), or null: the steps are the ring's
struct HostSteps {
    const uint16_t* step_move;
    const float* step_q;
    const uint32_t* child_off;   // [P + 1]
    const uint16_t* child_move;
    const int32_t* child_n;
    const float *child_q, *child_uct;
};

// one call: what the host knows of its games, and where that lives on the device
struct Job {
    int n = 0;
    std::vector<uint32_t> ply_src, ply_seg, seg_len, frame_off{0}, frame_seg;
    std::vector<uint32_t> first_ply{0}, first_seg{0};   // [n + 1]
    std::string blob;
    std::vector<uint64_t> text_off{0};                  // [n + 1], after count()
    uint32_t *d_ply_src = nullptr, *d_ply_seg = nullptr, *d_seg_len = nullptr, *d_seg_off = nullptr, *d_tile = nullptr, *d_total = nullptr,
             *d_frame_off = nullptr, *d_frame_seg = nullptr;
    char* d_blob = nullptr;
    sctw::Steps steps{};

    // a game of n_steps plies, read from step first_src on; the frames are the host writer's text around an empty "steps"
    int add_game(int n_steps, int has_outcome, int termination, int winner, const uint16_t* opening, int n_opening, const char* fen, uint32_t first_src) {
        static const char KEY[] = ",\n  \"steps\": ";
        const std::string frame = sctrace::trace_to_json(0, has_outcome, termination, winner, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                         opening, n_opening, fen);
        const size_t at = frame.find(std::string(KEY) + "[]");
        if (at == std::string::npos) return fail("trace writer: no \"steps\" in the frame");
        const size_t cut = at + sizeof KEY - 1;
        uint32_t seg = first_seg.back();
        auto add_frame = [&](const std::string& t) {
            blob += t;
            frame_off.push_back((uint32_t)blob.size());
            frame_seg.push_back(seg++);
            seg_len.push_back((uint32_t)t.size());
        };
        add_frame(frame.substr(0, cut) + (n_steps ? "[\n" : "[]"));
        for (int i = 0; i < n_steps; i++) {
            ply_src.push_back((first_src + (uint32_t)i) | (i + 1 == n_steps ? sctw::LAST_PLY : 0u));
            ply_seg.push_back(seg++);
            seg_len.push_back(0);
        }
        add_frame((n_steps ? "  ]" : "") + frame.substr(cut + 2));
        first_ply.push_back((uint32_t)ply_src.size());
        first_seg.push_back(seg);
        n++;
        return 0;
    }
};

template <class T>
int upload(T* d, const T* h, size_t count, hipStream_t st) {
    if (count) HIPOK(hipMemcpyAsync(d, h, count * sizeof(T), hipMemcpyHostToDevice, st));
    return 0;
}

int writer_open(TraceWriter& w) {
    if (!w.stream) HIPOK(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
    for (hipEvent_t& e : w.ev)
        if (!e) HIPOK(hipEventCreate(&e));
    return 0;
}

// The counting pass: everything the kernels read goes up, the lengths of the plies come back, text_off is filled.  ring: the
// steps are read in place (hs == nullptr)
int count(TraceWriter& w, Job& j, const HostSteps* hs, const sc::SpParams* ring) {
    TRY(writer_open(w));
    g_fmt_ms[0] = g_fmt_ms[1] = 0.f;
    j.text_off.assign((size_t)j.n + 1, 0);
    if (j.n == 0) return 0;
    const hipStream_t st = w.stream;
    const size_t P = j.ply_src.size(), S = j.seg_len.size(), F = j.frame_seg.size(), C = hs ? hs->child_off[P] : 0;
    uint16_t *d_move = nullptr, *d_cmove = nullptr;
    uint32_t *d_q = nullptr, *d_coff = nullptr, *d_cq = nullptr, *d_cu = nullptr;
    int32_t* d_cn = nullptr;
    ArenaLayout L;
    L.add(&j.d_ply_src, P);
    L.add(&j.d_ply_seg, P);
    L.add(&j.d_seg_len, S);
    L.add(&j.d_seg_off, S);
    L.add(&j.d_tile, (S + scl::SCAN_TILE - 1) / scl::SCAN_TILE);
    L.add(&j.d_total, 1);
    L.add(&j.d_frame_off, F + 1);
    L.add(&j.d_frame_seg, F);
    L.add(&j.d_blob, j.blob.size());
    L.add(&d_move, P, hs != nullptr);
    L.add(&d_q, P, hs != nullptr);
    L.add(&d_coff, P + 1, hs != nullptr);
    L.add(&d_cmove, C, hs != nullptr);
    L.add(&d_cn, C, hs != nullptr);
    L.add(&d_cq, C, hs != nullptr);
    L.add(&d_cu, C, hs != nullptr);
    TRY(w.arena.grow(L.bytes, [st] { return hipStreamSynchronize(st); }));
    L.bind(w.arena.p);
    TRY(upload(j.d_ply_src, j.ply_src.data(), P, st));
    TRY(upload(j.d_ply_seg, j.ply_seg.data(), P, st));
    TRY(upload(j.d_seg_len, j.seg_len.data(), S, st));
    TRY(upload(j.d_frame_off, j.frame_off.data(), F + 1, st));
    TRY(upload(j.d_frame_seg, j.frame_seg.data(), F, st));
    TRY(upload(j.d_blob, j.blob.data(), j.blob.size(), st));
    if (hs) {
        TRY(upload(d_move, hs->step_move, P, st));
        TRY(upload(d_q, reinterpret_cast<const uint32_t*>(hs->step_q), P, st));
        TRY(upload(d_coff, hs->child_off, P + 1, st));
        TRY(upload(d_cmove, hs->child_move, C, st));
        TRY(upload(d_cn, hs->child_n, C, st));
        TRY(upload(d_cq, reinterpret_cast<const uint32_t*>(hs->child_q), C, st));
        TRY(upload(d_cu, reinterpret_cast<const uint32_t*>(hs->child_uct), C, st));
        j.steps = sctw::Steps{d_move, d_q, d_coff, nullptr, d_cmove, d_cn, d_cq, d_cu};
    } else {
        j.steps = sctw::Steps{ring->t_move, reinterpret_cast<const uint32_t*>(ring->t_q), nullptr, ring->t_nchild, ring->t_cmove, ring->t_cn,
                              reinterpret_cast<const uint32_t*>(ring->t_cq), reinterpret_cast<const uint32_t*>(ring->t_cu)};
    }
    HIPOK(hipEventRecord(w.ev[0], st));
    scl::trace_write_count(sctw::Plies{(uint32_t)P, j.d_ply_src, j.d_ply_seg}, j.steps, j.d_seg_len, st);
    HIPOK(hipEventRecord(w.ev[1], st));
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(j.seg_len.data(), j.d_seg_len, S * 4, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    HIPOK(hipEventElapsedTime(&g_fmt_ms[0], w.ev[0], w.ev[1]));
    for (int g = 0; g < j.n; g++) {
        uint64_t bytes = 0;
        for (uint32_t s = j.first_seg[(size_t)g]; s < j.first_seg[(size_t)g + 1]; s++) bytes += j.seg_len[s];
        j.text_off[(size_t)g + 1] = j.text_off[(size_t)g] + bytes;
    }
    return 0;
}

// The emitting pass, after count(): the text of every game into host_text[text_off[g] ..), in groups of games below 2^31 bytes
int emit(TraceWriter& w, const Job& j, char* host_text) {
    const hipStream_t st = w.stream;
    for (int g0 = 0; g0 < j.n;) {
        int g1 = g0 + 1;
        while (g1 < j.n && j.text_off[(size_t)g1 + 1] - j.text_off[(size_t)g0] < GROUP_LIMIT) g1++;
        const uint64_t bytes = j.text_off[(size_t)g1] - j.text_off[(size_t)g0];
        if (bytes >= GROUP_LIMIT) return fail("trace writer: a single game of 2 GiB of text or more");
        const uint32_t s0 = j.first_seg[(size_t)g0], s1 = j.first_seg[(size_t)g1], p0 = j.first_ply[(size_t)g0], p1 = j.first_ply[(size_t)g1];
        TRY(w.text.grow((size_t)bytes + 16, [st] { return hipStreamSynchronize(st); }));
        HIPOK(hipEventRecord(w.ev[2], st));
        scl::exclusive_scan_u32(s1 - s0, j.d_seg_len + s0, j.d_tile, j.d_seg_off + s0, j.d_total, st);
        scl::trace_write_emit(sctw::Plies{p1 - p0, j.d_ply_src + p0, j.d_ply_seg + p0}, j.steps,
                              sctw::Frames{2u * (uint32_t)(g1 - g0), j.d_blob, j.d_frame_off + 2 * (size_t)g0, j.d_frame_seg + 2 * (size_t)g0},
                              sctw::Out{j.d_seg_off, w.text.p}, st);
        HIPOK(hipEventRecord(w.ev[3], st));
        HIPOK(hipGetLastError());
        if (bytes) HIPOK(hipMemcpyAsync(host_text + j.text_off[(size_t)g0], w.text.p, (size_t)bytes, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));   // (the next group reuses the text buffer and the scan's scratch)
        float ms = 0.f;
        HIPOK(hipEventElapsedTime(&ms, w.ev[2], w.ev[3]));
        g_fmt_ms[1] += ms;
        g0 = g1;
    }
    return 0;
}

// text == nullptr: the sizing call.  Nothing is written when cap is too small
int finish(TraceWriter& w, const Job& j, char* text, uint64_t cap, uint64_t* text_off) {
    if (text && j.text_off.back() > cap) return fail("trace writer: the text needs " + std::to_string(j.text_off.back()) + " bytes, cap is " + std::to_string(cap));
    std::copy(j.text_off.begin(), j.text_off.end(), text_off);
    return text ? emit(w, j, text) : 0;
}

// The ring rows of n requested games, with the readiness rules of sc_selfplay_encode_traces: 0 and the job, 1 / 2, < 0
int ring_job(sc_selfplay* sp, int n, const int32_t* games, Job& j) {
    if (!sp || n < 0 || (n > 0 && !games)) return fail("bad argument");
    if (sp->poisoned) return sp_refuse(sp);
    const sc::SpParams& p = sp->p;
    if ((uint64_t)p.trace_cap * (uint64_t)p.num_steps >= sctw::LAST_PLY) return fail("trace writer: the trace ring has 2^31 steps or more");
    std::vector<int32_t> rows((size_t)std::max(n, 1));
    bool all_held = true;
    for (int i = 0; i < n; i++) {
        const int g = games[i];
        if (g < 0 || g >= p.total_games) return fail("bad argument: game index out of range");
        rows[(size_t)i] = g % p.trace_cap;
        all_held = all_held && row_held(sp, rows[(size_t)i], p.first_game_id + (uint64_t)g);
    }
    // held rows are final: they are read while the handle's stream works on (the copy below is on the NULL stream, the launch
    // stream is non-blocking); anything else is read from an idle stream
    if (all_held) HIPOK(hipSetDevice(sp->device));
    else TRY(sp_quiesce(sp, true));
    std::vector<sc::TraceHdr> hdr((size_t)p.trace_cap);
    HIPOK(hipMemcpy(hdr.data(), p.thdr, hdr.size() * sizeof(sc::TraceHdr), hipMemcpyDeviceToHost));
    int not_finished = 0, gone = 0;
    for (int i = 0; i < n; i++) {
        const RowState rs = row_state(sp, rows[(size_t)i], p.first_game_id + (uint64_t)games[i], hdr[(size_t)rows[(size_t)i]]);
        gone |= rs == ROW_GONE;
        not_finished |= rs == ROW_NOT_FINISHED;
    }
    if (gone) return fail("trace released or overwritten (trace_capacity ring)", 2);
    if (not_finished) return fail("game not finished", 1);
    for (int i = 0; i < n; i++) {
        const sc::TraceHdr& h = hdr[(size_t)rows[(size_t)i]];
        const uint16_t* line = nullptr;
        const int len = sp_opening(sp, games[i], &line);
        TRY(j.add_game(std::min(std::max(h.n_steps, 0), p.num_steps), h.has_outcome, h.termination, h.winner, line, len, sp_opening_fen(sp, games[i]),
                       (uint32_t)rows[(size_t)i] * (uint32_t)p.num_steps));
    }
    if (!sp->writer) sp->writer = new TraceWriter();
    return count(*sp->writer, j, nullptr, &p);
}

}  // namespace

extern "C" {

int sc_trace_format_f32(int n, const float* v, char* text, uint8_t* len) {
    if (n < 0 || (n > 0 && (!v || !text || !len))) return fail("bad argument");
    for (int i = 0; i < n; i++) {
        uint32_t bits;
        memcpy(&bits, v + i, 4);
        scfmt::BufSink s{text + (size_t)i * scfmt::F32_MAX_TEXT};
        scfmt::fmt_f32(s, bits);
        len[i] = (uint8_t)s.n;
    }
    return 0;
}

int sc_traces_format(int device_id, int n, const sc_trace_info* info, const uint32_t* step_off, const uint16_t* step_move, const float* step_q,
                     const uint32_t* child_off, const uint16_t* child_move, const int32_t* child_n, const float* child_q, const float* child_uct,
                     const uint32_t* open_off, const uint16_t* opening, const char* const* fens, char* text, uint64_t cap, uint64_t* text_off) {
    if (n < 0 || !text_off || (n > 0 && (!info || !step_off || !child_off))) return fail("bad argument");
    if (n > 0) {
        TRY(check_traces(n, step_off, child_off));
        if (step_off[0] != 0 || child_off[0] != 0) return fail("sc_traces_format: step_off[0] and child_off[0] must be 0");
        if (step_off[n] >= sctw::LAST_PLY) return fail("sc_traces_format: 2^31 steps or more in one call");
        if (step_off[n] > 0 && (!step_move || !step_q)) return fail("bad argument");
        if (child_off[step_off[n]] > 0 && (!child_move || !child_n || !child_q || !child_uct)) return fail("bad argument");
        for (int g = 0; g < n; g++) {
            if (info[g].n_steps < 0 || (uint32_t)info[g].n_steps != step_off[g + 1] - step_off[g])
                return fail("sc_traces_format: info[" + std::to_string(g) + "].n_steps differs from step_off");
            if (open_off && open_off[g + 1] < open_off[g]) return fail("sc_traces_format: open_off is not monotonic");
        }
        if (open_off && open_off[n] > open_off[0] && !opening) return fail("bad argument");
    }
    TRY(use_device(nullptr, device_id));
    Job j;
    for (int g = 0; g < n; g++)
        TRY(j.add_game(info[g].n_steps, info[g].has_outcome, info[g].termination, info[g].winner, open_off ? opening + open_off[g] : nullptr,
                       open_off ? (int)(open_off[g + 1] - open_off[g]) : 0, fens ? fens[g] : nullptr, step_off[g]));
    TraceWriter w;
    const HostSteps hs{step_move, step_q, child_off, child_move, child_n, child_q, child_uct};
    TRY(count(w, j, &hs, nullptr));
    return finish(w, j, text, cap, text_off);
}

int sc_selfplay_traces_json(sc_selfplay* sp, int n, const int32_t* games, char* text, uint64_t cap, uint64_t* text_off) {
    if (!text_off) return fail("bad argument");
    Job j;
    TRY(ring_job(sp, n, games, j));
    return finish(*sp->writer, j, text, cap, text_off);
}

int sc_selfplay_write_traces_json(sc_selfplay* sp, int n, const int32_t* games, const char* const* paths) {
    if (n > 0 && !paths) return fail("bad argument");
    for (int i = 0; i < n; i++)
        if (!paths[i]) return fail("bad argument");
    Job j;
    TRY(ring_job(sp, n, games, j));
    TraceWriter& w = *sp->writer;
    const size_t bytes = (size_t)j.text_off.back();
    if (bytes > w.pinned_cap) {
        if (w.pinned) HIPOK(hipHostFree(w.pinned));
        w.pinned = nullptr;
        w.pinned_cap = 0;
        const size_t want = std::max(bytes + bytes / 2, (size_t)1 << 20);
        HIPOK(hipHostMalloc(reinterpret_cast<void**>(&w.pinned), want, hipHostMallocDefault));
        w.pinned_cap = want;
    }
    TRY(emit(w, j, w.pinned));
    for (int i = 0; i < n; i++) {
        FILE* f = fopen(paths[i], "wb");
        if (!f) return fail(std::string("cannot open ") + paths[i]);
        const size_t len = (size_t)(j.text_off[(size_t)i + 1] - j.text_off[(size_t)i]);
        const size_t wr = fwrite(w.pinned + j.text_off[(size_t)i], 1, len, f);
        fclose(f);
        if (wr != len) return fail("short write");
    }
    return 0;
}

int sc_traces_format_last_timing(float* count_ms, float* emit_ms) {
    if (count_ms) *count_ms = g_fmt_ms[0];
    if (emit_ms) *emit_ms = g_fmt_ms[1];
    return 0;
}

}  // extern "C"
