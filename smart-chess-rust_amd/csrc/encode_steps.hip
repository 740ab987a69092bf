// encode_steps.hip -- host side of libsc_engine.so: training tensors (sc_encode_steps, sc_encode_steps_device, sc_encode_san_device,
// sc_traces_encode_device)
// and, on the same walk and arena, moves written as SAN (sc_moves_to_san_device, sc_san_format).
//
// libsmartchess.chess_encode_steps (reference src/lib.rs:46-128) for a batch of recorded games; see include/sc_engine.h.
// One encoder, encode_device_core, writes device buffers on a stream from a described source (EncodeSrc); it and san_write_core
// share one set-up, GameBatch.  sc_encode_steps_device / sc_selfplay_encode_traces hand it the caller's buffers and stream: nothing
// is staged or waits for the device in the steady state.  sc_encode_steps runs it into staging, slice by slice, and copies out.
// The scratch of a call lives in a per-device arena that the library keeps and reuses: an event recorded behind each call's
// work orders the next call after it on the device (hipStreamWaitEvent, whatever its stream); only growing the arena waits
// on the host, for that previous call, before the old buffer is freed.
#include <chrono>
#include <map>
#include <mutex>

#include "host_common.hpp"
#include "san_tokens.hpp"

static thread_local float g_encode_ms[2] = {0.f, 0.f};   // last sc_encode_steps of this thread: kernels (HIP events), whole call

namespace {
struct EncArena {
    DevBuf<char> buf;
    hipEvent_t ev = nullptr;   // behind the last call's work
    bool used = false;
};
std::mutex g_enc_mu;   // held across a call's enqueue: calls on one device take the arena in turn
std::map<int, EncArena> g_enc_arena;
struct ArenaRelease {   // scope guard: on every path out of the call (failures included), later calls wait for what was enqueued
    std::unique_lock<std::mutex> lk;   // (released behind the event's record)
    EncArena* a = nullptr;             // set once the arena is taken, with the call's stream
    hipStream_t s = nullptr;
    ~ArenaRelease() { if (a && hipEventRecord(a->ev, s) == hipSuccess) a->used = true; }
};
}  // namespace

// output pointers must be device memory of `dev` (a host pointer, or memory of another GPU, would be written by kernels that
// cannot reach it)
static int check_device_ptr(const void* ptr, int dev, const char* name) {
    if (!ptr) return 0;
    hipPointerAttribute_t a{};
    const hipError_t e = hipPointerGetAttributes(&a, ptr);
    (void)hipGetLastError();   // (an unknown host pointer is an error of this query only)
    if (e != hipSuccess || a.type != hipMemoryTypeDevice)
        return fail(std::string(name) + ": not device memory (outputs of this call are device pointers, e.g. hipMalloc or a torch "
                    "tensor on the handle's GPU)");
    if (a.device != dev)
        return fail(std::string(name) + ": memory of device " + std::to_string(a.device) + ", the call runs on device " + std::to_string(dev));
    return 0;
}

int check_device_ptrs(std::initializer_list<std::pair<const void*, const char*>> ptrs, int dev) {
    for (const auto& x : ptrs) TRY(check_device_ptr(x.first, dev, x.second));
    return 0;
}
int check_device_outputs(const DevEncodeOut& o, int dev) {
    if (o.layout != 0 && o.layout != 1) return fail("layout must be 0 (reference) or 1 (trainer)");
    return check_device_ptrs({{o.boards, "boards"}, {o.meta, "meta"}, {o.dist, "dist"}, {o.dist_legal, "dist_legal"},
                              {o.legal_idx, "legal_idx"}, {o.n_legal, "n_legal"}, {o.status, "status"}}, dev);
}

namespace {
// the game records of one group of games: (games in the group) x (longest game of the group + 2) <= REC_BUDGET, so one long
// game among many short ones does not size the buffer for all of them (80 B per record: 80 MiB)
struct Group { int g0, ng, hist_cap; };
std::vector<Group> record_groups(int n_games, const uint32_t* ply_off, size_t* max_rec) {
    const size_t REC_BUDGET = (size_t)1 << 20;
    std::vector<Group> groups;
    *max_rec = 1;
    for (int g0 = 0; g0 < n_games;) {
        uint32_t mx = ply_off[g0 + 1] - ply_off[g0];
        int g1 = g0 + 1;
        while (g1 < n_games) {
            const uint32_t m2 = std::max(mx, ply_off[g1 + 1] - ply_off[g1]);
            if ((size_t)(g1 - g0 + 1) * (m2 + 2) > REC_BUDGET) break;
            mx = m2;
            g1++;
        }
        groups.push_back({g0, g1 - g0, (int)mx + 2});
        *max_rec = std::max(*max_rec, (size_t)(g1 - g0) * (mx + 2));
        g0 = g1;
    }
    return groups;
}
// What every call that walks recorded games sets up (encode_device_core, san_write_core): the record groups, the arena regions all
// of them use -- a core adds its own to L before open() -- the arena, taken in turn and released behind the call's work, the uploads
// of the offsets and base indices, the fill of the games' status keys (status_fill or null), per group the ply index and the walk.
struct GameBatch {
    const int n_games;
    const uint32_t* const ply_off;   // host, n_games + 1 (the plies of game g are [ply_off[g], ply_off[g+1]))
    const uint32_t P;
    const hipStream_t st;
    const HostBases host;
    std::vector<Group> groups;
    ArenaLayout L;
    uint32_t* d_off;
    uint16_t* d_moves;   // [P]: the source's upload, parse or ring copy
    sc::PlyIndex idx;
    sc::Position* d_hist;
    int32_t* d_bidx;
    sc::Bases bases{nullptr, nullptr};   // on the device, once open
    ArenaRelease release;
    GameBatch(int n_games_, const uint32_t* ply_off_, const HostBases& b, hipStream_t st_)
        : n_games(n_games_), ply_off(ply_off_), P(ply_off_[n_games_]), st(st_), host(b) {
        size_t max_rec = 1;
        groups = record_groups(n_games, ply_off, &max_rec);
        L.add(&d_off, (size_t)n_games + 1);
        L.add(&d_moves, (size_t)P);
        L.add(&idx.hoff, (size_t)P);
        L.add(&idx.plen, (size_t)P);
        L.add(&idx.pgame, (size_t)P);
        L.add(&d_hist, max_rec);
        L.add(&d_bidx, (size_t)n_games, b.rec != nullptr);
    }
    int open(int dev) {
        release.lk = std::unique_lock<std::mutex>(g_enc_mu);
        EncArena& A = g_enc_arena[dev];   // the device's arena: grown if need be, ordered behind the previous call
        if (!A.ev) HIPOK(hipEventCreateWithFlags(&A.ev, hipEventDisableTiming));
        if (L.bytes > A.buf.cap) {
            // the previous call's work still reads the old arena
            TRY(A.buf.grow(L.bytes, [&A] { return A.used ? hipEventSynchronize(A.ev) : hipSuccess; }));
            A.used = false;
        } else if (A.used) {
            HIPOK(hipStreamWaitEvent(st, A.ev, 0));   // ... possibly on another stream
        }
        release.a = &A;
        release.s = st;
        L.bind(A.buf.p);
        HIPOK(hipMemcpyAsync(d_off, ply_off, ((size_t)n_games + 1) * 4, hipMemcpyHostToDevice, st));
        bases = {host.rec, d_bidx};
        if (host.rec) HIPOK(hipMemcpyAsync(d_bidx, host.idx, (size_t)n_games * 4, hipMemcpyHostToDevice, st));
        return 0;
    }
    // per group with plies [p0, p1): the index, the walk (with_keys: and the plies' keys and repetition flags), then per_ply(p0, p1)
    template <class PerPly>
    int each_group(const sc::RingPlies& ring, bool with_keys, int32_t* status_fill, PerPly per_ply) {
        if (status_fill) HIPOK(hipMemsetAsync(status_fill, sc::STATUS_FILL_BYTE, (size_t)n_games * 4, st));   // behind the source's uploads
        for (const Group& gr : groups) {
            const uint32_t p0 = ply_off[gr.g0], p1 = ply_off[gr.g0 + gr.ng];
            if (p1 == p0) continue;
            scl::ply_index({(int)(p1 - p0), gr.g0, gr.ng, d_off, gr.hist_cap}, idx, ring, st);
            const sc::GameWalk w{gr.ng, d_moves, d_off + gr.g0, d_hist, gr.hist_cap, bases.from(gr.g0)};
            if (with_keys) scl::replay_games(w, (int)(p1 - p0), idx.from(p0), d_moves + p0, st);
            else scl::replay_walk(w, st);
            TRY(per_ply(p0, p1));
        }
        return 0;
    }
};
}  // namespace

// One encoder for the four kinds of source (EncodeSrc, host_common.hpp).  In the SAN kind k_san_parse also writes the games'
// status, and the parsed moves stay in the arena between the two halves: nothing comes back to the host.
int encode_device_core(int dev, int n_games, const uint32_t* ply_off, const EncodeSrc& src, int apply_mirror, const DevEncodeOut& o,
                       hipStream_t st) {
    const bool has_ring = src.kind == EncodeSrc::RING, has_csr = src.kind == EncodeSrc::CSR, has_san = src.kind == EncodeSrc::SAN;
    const bool has_dev = src.kind == EncodeSrc::DEV;
    GameBatch B(n_games, ply_off, src.bases, st);
    const uint32_t P = B.P, CH = 32768;   // CH: plies per launch of the per-ply kernels (bounds their legal-move / meta scratch: 15 MB)
    const uint32_t nchild = has_csr ? src.child_off[P] : 0, cap = std::max<uint32_t>(std::min(CH, P), 1);
    uint32_t *d_src, *d_coff, *d_cn;
    uint16_t *d_lm, *d_cmv;
    uint64_t* d_tok;
    int32_t *d_meta, *d_nl, *d_rows;
    B.L.add(&d_lm, (size_t)cap * 224);
    B.L.add(&d_meta, (size_t)cap * 7);
    B.L.add(&d_nl, (size_t)cap);
    B.L.add(&d_rows, (size_t)n_games, has_ring);
    B.L.add(&d_src, (size_t)P, has_ring);
    B.L.add(&d_coff, (size_t)P + 1, has_csr);
    B.L.add(&d_cmv, (size_t)nchild, has_csr);
    B.L.add(&d_cn, (size_t)nchild, has_csr);
    B.L.add(&d_tok, (size_t)P, has_san);
    TRY(B.open(dev));
    sc::RingPlies ring{};
    sc::Children ch{};
    if (has_ring) {
        HIPOK(hipMemcpyAsync(d_rows, src.rows, (size_t)n_games * 4, hipMemcpyHostToDevice, st));
        ring = {d_rows, src.p->num_steps, src.p->t_move, B.d_moves, d_src};
        ch = {src.p->t_cmove, reinterpret_cast<const uint32_t*>(src.p->t_cn), nullptr, d_src, src.p->t_nchild};
    } else if (has_san) {
        if (P) HIPOK(hipMemcpyAsync(d_tok, src.tokens, (size_t)P * 8, hipMemcpyHostToDevice, st));
        scl::san_parse(n_games, d_tok, B.d_off, B.d_moves, o.status, B.bases, st);
        if (P && src.moves_out) HIPOK(hipMemcpyAsync(src.moves_out, B.d_moves, (size_t)P * 2, hipMemcpyDeviceToDevice, st));
    } else if (has_dev) {   // the moves into the batch, the children read where the parsed set keeps them
        if (P) HIPOK(hipMemcpyAsync(B.d_moves, src.moves, (size_t)P * 2, hipMemcpyDeviceToDevice, st));
        ch = {src.child_mv, src.child_n, src.child_off, nullptr, nullptr};
    } else {
        if (P) HIPOK(hipMemcpyAsync(B.d_moves, src.moves, (size_t)P * 2, hipMemcpyHostToDevice, st));
        HIPOK(hipMemcpyAsync(d_coff, src.child_off, ((size_t)P + 1) * 4, hipMemcpyHostToDevice, st));
        if (nchild) {
            HIPOK(hipMemcpyAsync(d_cmv, src.child_mv, (size_t)nchild * 2, hipMemcpyHostToDevice, st));
            HIPOK(hipMemcpyAsync(d_cn, src.child_n, (size_t)nchild * 4, hipMemcpyHostToDevice, st));
        }
        ch = {d_cmv, d_cn, d_coff, nullptr, nullptr};
    }
    const size_t bsz = o.layout == 1 ? 4 : 1, msz = 4;
    const bool rows_wanted = o.boards || o.meta || o.dist || o.dist_legal || o.legal_idx || o.n_legal;
    if (!has_san || rows_wanted)   // (else SAN -> moves alone)
        TRY(B.each_group(ring, true, has_san ? nullptr : o.status, [&](uint32_t p0, uint32_t p1) {
            for (uint32_t c0 = p0; c0 < p1; c0 += CH) {
                const uint32_t n = std::min(CH, p1 - c0);
                scl::encode_plies(o.layout, (int)n, B.d_hist, B.idx.from(c0),
                                  {o.boards ? static_cast<char*>(o.boards) + (size_t)c0 * 7168 * bsz : nullptr, d_meta, d_lm,
                                   o.legal_idx ? o.legal_idx + (size_t)c0 * 224 : nullptr, d_nl}, st);
                const sc::PlyMoves pm{d_lm, d_nl, B.d_moves + c0};
                const sc::RowOut rows{apply_mirror, d_meta, o.layout, o.meta ? static_cast<char*>(o.meta) + (size_t)c0 * 7 * msz : nullptr,
                                      o.dist ? o.dist + (size_t)c0 * 4672 : nullptr, o.dist_legal ? o.dist_legal + (size_t)c0 * 224 : nullptr,
                                      o.n_legal ? o.n_legal + c0 : nullptr};
                if (has_san) scl::san_dist((int)n, pm, rows, st);
                else scl::steps_dist((int)n, pm, ch.from(c0), B.idx.from(c0), rows, o.status, st);
            }
            return 0;
        }));
    if (!has_san) scl::status_final(n_games, o.status, st);
    if (has_dev) scl::trace_status(n_games, src.over, o.status, st);
    HIPOK(hipGetLastError());
    return 0;
}

// sc_moves_to_san_device on the same set-up: per group the index and the walk alone (a move generation reads neither keys nor
// repetition flags), then one wavefront per ply (k_san_write).  The status keys are k_steps_dist's, the tokens behind a game's
// first failing ply are zeroed before k_status_final turns the keys into codes.
static int san_write_core(int dev, int n_games, const uint32_t* ply_off, const uint16_t* moves, const HostBases& bases, uint64_t* tokens,
                          int32_t* status, hipStream_t st) {
    GameBatch B(n_games, ply_off, bases, st);
    TRY(B.open(dev));
    if (B.P) HIPOK(hipMemcpyAsync(B.d_moves, moves, (size_t)B.P * 2, hipMemcpyHostToDevice, st));
    TRY(B.each_group(sc::RingPlies{}, false, status, [&](uint32_t p0, uint32_t p1) {
        scl::san_write((int)(p1 - p0), B.d_hist, B.idx.from(p0), B.d_moves + p0, tokens + p0, status, st);
        return 0;
    }));
    scl::san_clip((int)B.P, B.idx, status, tokens, st);
    scl::status_final(n_games, status, st);
    HIPOK(hipGetLastError());
    return 0;
}

int check_traces(int n_games, const uint32_t* move_off, const uint32_t* child_off) {
    uint32_t maxlen = 0;
    for (int g = 0; g < n_games; g++) {
        if (move_off[g + 1] < move_off[g]) return fail("move_off not monotonic");
        maxlen = std::max(maxlen, move_off[g + 1] - move_off[g]);
    }
    if (maxlen > 4000) return fail("move list too long");
    for (uint32_t p = 0; child_off && p < move_off[n_games]; p++)
        if (child_off[p + 1] < child_off[p] || child_off[p + 1] - child_off[p] > 224) return fail("child_off: more than 224 children or not monotonic");
    return 0;
}

// the opening of the three *_device_from entry points behind their null checks: the device of the call and its bases
struct DeviceCall { int dev; HostBases bases; };
static int device_call_open(const sc_engine* e, int device_id, int n_games, const sc_positions* bases, const int32_t* base_idx, const char* who, DeviceCall* c) {
    TRY(use_device(e, device_id));
    *c = {e ? e->device : device_id, {nullptr, base_idx}};
    return positions_bases(bases, base_idx, n_games, c->dev, false, who, &c->bases.rec);
}

extern "C" {

int sc_encode_steps_device(sc_engine* e, int device_id, int n_games, const uint16_t* moves, const uint32_t* move_off,
                           const uint16_t* child_mv, const uint32_t* child_n, const uint32_t* child_off, int apply_mirror, int layout,
                           void* stream, void* boards, void* meta, float* dist, float* dist_legal, uint16_t* legal_idx,
                           int32_t* n_legal, int32_t* status) {
    return sc_encode_steps_device_from(e, device_id, n_games, nullptr, nullptr, moves, move_off, child_mv, child_n, child_off, apply_mirror,
                                       layout, stream, boards, meta, dist, dist_legal, legal_idx, n_legal, status);
}

int sc_encode_steps_device_from(sc_engine* e, int device_id, int n_games, const sc_positions* bases, const int32_t* base_idx,
                                const uint16_t* moves, const uint32_t* move_off, const uint16_t* child_mv, const uint32_t* child_n,
                                const uint32_t* child_off, int apply_mirror, int layout, void* stream, void* boards, void* meta,
                                float* dist, float* dist_legal, uint16_t* legal_idx, int32_t* n_legal, int32_t* status) {
    if (n_games < 0 || !move_off || !child_off || !status) return fail("bad argument");
    const DevEncodeOut o{layout, boards, meta, dist, dist_legal, legal_idx, n_legal, status};
    DeviceCall c;
    TRY(device_call_open(e, device_id, n_games, bases, base_idx, "sc_encode_steps_device_from", &c));
    TRY(check_device_outputs(o, c.dev));
    if (n_games == 0) return 0;
    TRY(check_traces(n_games, move_off, child_off));
    const uint32_t total = move_off[n_games];
    if (total && !moves) return fail("bad argument");
    if (child_off[total] && (!child_mv || !child_n)) return fail("bad argument");
    return encode_device_core(c.dev, n_games, move_off, EncodeSrc::csr(moves, child_mv, child_n, child_off, c.bases), apply_mirror, o,
                              static_cast<hipStream_t>(stream));
}

int sc_encode_san_device(sc_engine* e, int device_id, int n_games, const uint64_t* tokens, const uint32_t* tok_off, int apply_mirror,
                         int layout, void* stream, void* boards, void* meta, float* dist, float* dist_legal, uint16_t* legal_idx,
                         int32_t* n_legal, uint16_t* moves, int32_t* status) {
    return sc_encode_san_device_from(e, device_id, n_games, nullptr, nullptr, tokens, tok_off, apply_mirror, layout, stream, boards, meta, dist,
                                     dist_legal, legal_idx, n_legal, moves, status);
}

int sc_encode_san_device_from(sc_engine* e, int device_id, int n_games, const sc_positions* bases, const int32_t* base_idx,
                              const uint64_t* tokens, const uint32_t* tok_off, int apply_mirror, int layout, void* stream, void* boards,
                              void* meta, float* dist, float* dist_legal, uint16_t* legal_idx, int32_t* n_legal, uint16_t* moves,
                              int32_t* status) {
    if (n_games < 0 || !tok_off || !status) return fail("bad argument");
    const DevEncodeOut o{layout, boards, meta, dist, dist_legal, legal_idx, n_legal, status};
    DeviceCall c;
    TRY(device_call_open(e, device_id, n_games, bases, base_idx, "sc_encode_san_device_from", &c));
    TRY(check_device_outputs(o, c.dev));
    TRY(check_device_ptrs({{moves, "moves"}}, c.dev));
    if (n_games == 0) return 0;
    TRY(check_traces(n_games, tok_off, nullptr));
    if (tok_off[n_games] && !tokens) return fail("bad argument");
    return encode_device_core(c.dev, n_games, tok_off, EncodeSrc::san(tokens, moves, c.bases), apply_mirror, o, static_cast<hipStream_t>(stream));
}

int sc_traces_encode_device(sc_engine* e, const sc_traces* t, int g0, int n, int apply_mirror, int layout, void* stream, void* boards,
                            void* meta, float* dist, float* dist_legal, uint16_t* legal_idx, int32_t* n_legal, int32_t* status) {
    if (!t || g0 < 0 || n < 0 || (int64_t)g0 + n > t->n || !status) return fail("bad argument");
    const DevEncodeOut o{layout, boards, meta, dist, dist_legal, legal_idx, n_legal, status};
    TRY(use_device(e, t->device));
    if (e && e->device != t->device)
        return fail("sc_traces_encode_device: the traces live on device " + std::to_string(t->device) + ", the engine on device " + std::to_string(e->device));
    TRY(check_device_outputs(o, t->device));
    if (n == 0) return 0;
    const uint32_t p0 = t->move_off[(size_t)g0];
    return encode_device_core(t->device, n, traces_range_off(t, g0),
                              EncodeSrc::dev(t->d_moves + p0, t->d_child_mv, t->d_child_n, t->d_child_off + p0, t->d_over + g0), apply_mirror, o,
                              static_cast<hipStream_t>(stream));
}

int sc_moves_to_san_device(int device_id, int n_games, const uint16_t* moves, const uint32_t* move_off, void* stream, uint64_t* tokens,
                           int32_t* status) {
    return sc_moves_to_san_device_from(device_id, n_games, nullptr, nullptr, moves, move_off, stream, tokens, status);
}

int sc_moves_to_san_device_from(int device_id, int n_games, const sc_positions* bases, const int32_t* base_idx, const uint16_t* moves,
                                const uint32_t* move_off, void* stream, uint64_t* tokens, int32_t* status) {
    if (n_games < 0 || !move_off || !status || !tokens) return fail("bad argument");
    DeviceCall c;
    TRY(device_call_open(nullptr, device_id, n_games, bases, base_idx, "sc_moves_to_san_device_from", &c));
    TRY(check_device_ptrs({{tokens, "tokens"}, {status, "status"}}, c.dev));
    if (n_games == 0) return 0;
    TRY(check_traces(n_games, move_off, nullptr));
    if (move_off[n_games] && !moves) return fail("bad argument");
    return san_write_core(c.dev, n_games, move_off, moves, c.bases, tokens, status, static_cast<hipStream_t>(stream));
}

int sc_san_tokenize(const char* text, size_t len, uint64_t* tokens, uint32_t cap, uint32_t* n_tokens) {
    if ((!text && len) || (!tokens && cap) || !n_tokens) return fail("bad argument");
    const size_t n = scsan::san_tokenize(text, len, tokens, cap);
    *n_tokens = (uint32_t)std::min<size_t>(n, UINT32_MAX);
    if (n > cap) return fail("sc_san_tokenize: " + std::to_string(n) + " tokens, room for " + std::to_string(cap), SC_ERR_CAPACITY);
    return 0;
}

int sc_san_format(const uint64_t* tokens, uint32_t n, int fullmove, int black_first, const char* result, char* buf, size_t cap) {
    if ((!tokens && n) || (!buf && cap) || fullmove < 0) return fail("bad argument");
    return (int)scsan::san_format(tokens, n, (unsigned)fullmove, black_first != 0, result, buf, cap);
}

namespace {
struct EncStaging {   // sc_encode_steps's device staging and timing events: released on every path out of the call
    ScopedDev<char> buf;
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~EncStaging() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};
}  // namespace

// the host-pointer form: encode_device_core (layout 0) into staging, slice by slice, and out through PCIe
int sc_encode_steps(sc_engine* e, int device_id, int n_games, const uint16_t* moves, const uint32_t* move_off,
                    const uint16_t* child_mv, const uint32_t* child_n, const uint32_t* child_off, int apply_mirror, int8_t* boards,
                    int32_t* meta, float* dist, uint16_t* legal_idx, int32_t* n_legal, int32_t* status) {
    if (n_games < 0 || !move_off || !child_off || !status) return fail("bad argument");
    if (n_games == 0) return 0;
    const auto t_call = std::chrono::steady_clock::now();
    TRY(use_device(e, device_id));
    const int dev = e ? e->device : device_id;
    std::fill(status, status + n_games, 0);
    TRY(check_traces(n_games, move_off, child_off));
    const uint32_t total = move_off[n_games];
    if (total == 0) return 0;
    // a slice: consecutive whole games of at most CH plies together (one game alone has at most 4000), which bounds the staging
    // at CH * 26 KB when every output is asked for
    const uint32_t CH = 8192, cap = std::min(CH, total);
    int32_t *d_status, *d_nl;
    char *d_boards, *d_meta;
    float* d_dist;
    uint16_t* d_li;
    ArenaLayout L;   // (an output the caller does not ask for is not staged)
    L.add(&d_status, (size_t)n_games);
    L.add(&d_boards, (size_t)cap * 7168, boards != nullptr);
    L.add(&d_meta, (size_t)cap * 28, meta != nullptr);
    L.add(&d_dist, (size_t)cap * 4672, dist != nullptr);
    L.add(&d_li, (size_t)cap * 224, legal_idx != nullptr);
    L.add(&d_nl, (size_t)cap, n_legal != nullptr);
    EncStaging S;
    HIPOK(S.buf.alloc(L.bytes));
    HIPOK(hipEventCreate(&S.ev[0]));
    HIPOK(hipEventCreate(&S.ev[1]));
    L.bind(S.buf.p);
    const hipStream_t st = e ? e->stream : nullptr;
    std::vector<uint32_t> moff, coff;   // the slice's offsets, rebased; uploaded asynchronously: alive until the slice's synchronisation
    float kernels_ms = 0.f;
    for (int g0 = 0, g1; g0 < n_games; g0 = g1) {
        const uint32_t p0 = move_off[g0], c0 = child_off[p0];
        for (g1 = g0 + 1; g1 < n_games && move_off[g1 + 1] - p0 <= CH; g1++) {}
        const uint32_t n = move_off[g1] - p0;
        moff.assign(move_off + g0, move_off + g1 + 1);
        coff.assign(child_off + p0, child_off + p0 + n + 1);
        for (uint32_t& x : moff) x -= p0;
        for (uint32_t& x : coff) x -= c0;
        const DevEncodeOut o{0, d_boards, d_meta, d_dist, nullptr, d_li, d_nl, d_status + g0};
        HIPOK(hipEventRecord(S.ev[0], st));
        TRY(encode_device_core(dev, g1 - g0, moff.data(), EncodeSrc::csr(moves + p0, child_mv + c0, child_n + c0, coff.data(), HostBases{}), apply_mirror, o, st));
        HIPOK(hipEventRecord(S.ev[1], st));
        HIPOK(hipStreamSynchronize(st));
        float ms = 0.f;
        HIPOK(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
        kernels_ms += ms;
        if (boards) HIPOK(hipMemcpy(boards + (size_t)p0 * 7168, o.boards, (size_t)n * 7168, hipMemcpyDeviceToHost));
        if (meta) HIPOK(hipMemcpy(meta + (size_t)p0 * 7, o.meta, (size_t)n * 28, hipMemcpyDeviceToHost));
        if (dist) HIPOK(hipMemcpy(dist + (size_t)p0 * 4672, o.dist, (size_t)n * 4672 * 4, hipMemcpyDeviceToHost));
        if (legal_idx) HIPOK(hipMemcpy(legal_idx + (size_t)p0 * 224, o.legal_idx, (size_t)n * 448, hipMemcpyDeviceToHost));
        if (n_legal) HIPOK(hipMemcpy(n_legal + p0, o.n_legal, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    HIPOK(hipMemcpy(status, d_status, (size_t)n_games * 4, hipMemcpyDeviceToHost));
    g_encode_ms[0] = kernels_ms;
    g_encode_ms[1] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_call).count();
    return 0;
}

int sc_encode_steps_last_timing(float* kernels_ms, float* total_ms) {
    if (kernels_ms) *kernels_ms = g_encode_ms[0];
    if (total_ms) *total_ms = g_encode_ms[1];
    return 0;
}

}  // extern "C"
