// host_common.hpp -- what the host units of libsc_engine.so share (engine.hip, encode_steps.hip, device_calls.hip, selfplay.hip,
// match_play.hip, selfplay_io.hip, report.hip, advance.hip, debug_calls.hip): error state, the handles' structs, the described source of an encode
// (EncodeSrc) and one helper for each piece of plumbing.  Host only: no kernel unit includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <assert.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/sc_engine.h"
#include "launchers.hpp"

#pragma GCC visibility push(hidden)   // internal to the library: only the C ABI is exported

// ------------------------------------------------------------------ errors
extern thread_local std::string g_err;   // sc_last_error() of this thread (engine.hip)
int fail(const std::string& m, int code = -1);
#define HIPOK(expr)                                                                                   \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_), -2);     \
    } while (0)
// a call that has already reported its failure (fail / HIPOK): pass its return code on
#define TRY(expr)                    \
    do {                             \
        const int rc_ = (expr);      \
        if (rc_) return rc_;         \
    } while (0)

// ------------------------------------------------------------------ device memory
template <class T>
static hipError_t dalloc(T** p, size_t n) {
    return hipMalloc(reinterpret_cast<void**>(p), std::max<size_t>(n, 1) * sizeof(T));
}
// cleanup paths: free a list of device pointers, ignoring errors
static inline void dfree(std::initializer_list<void*> ptrs) {
    for (void* q : ptrs)
        if (q) (void)hipFree(q);
}

// "no HIP device" (-3), "device_id out of range" (-1), hipSetDevice: the opening of every call that names its device, which is
// the engine's if there is one, else device_id.  The engine is not looked at before a device has been found.
int use_device(const sc_engine* e, int device_id);

// a call-local device buffer, freed on every path out of the call
template <class T>
struct ScopedDev {
    T* p = nullptr;
    ScopedDev() = default;
    ScopedDev(const ScopedDev&) = delete;
    ScopedDev& operator=(const ScopedDev&) = delete;
    ~ScopedDev() { dfree({p}); }
    hipError_t alloc(size_t n) { return dalloc(&p, n); }
};

// a device buffer that is kept and grown on demand (cap in elements).  Growing frees the old buffer: wait() is called first and
// returns once nothing on the device uses it any more.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    template <class Wait>
    int grow(size_t want, Wait wait) {
        if (want <= cap) return 0;
        HIPOK(wait());
        release();
        HIPOK(dalloc(&p, want));
        cap = want;
        return 0;
    }
    void release() {
        dfree({p});
        p = nullptr;
        cap = 0;
    }
};

// The regions of one device allocation.  add() registers a pointer and the elements it needs, bytes is then the size to
// allocate, bind() points every registered pointer into the block.  Regions start 256 bytes apart at least and hold one byte at
// least; a region that is not wanted takes no room and its pointer stays null.
struct ArenaLayout {
    struct Region {
        void* slot;
        size_t off;
        void (*set)(void* slot, char* at);
    };
    Region regions[16];
    int n = 0;
    size_t bytes = 0;
    template <class T>
    void add(T** slot, size_t count, bool wanted = true) {
        *slot = nullptr;
        if (!wanted) return;
        assert(n < 16);
        regions[n++] = {slot, bytes, [](void* s, char* at) { *static_cast<T**>(s) = reinterpret_cast<T*>(at); }};
        bytes += (std::max<size_t>(count * sizeof(T), 1) + 255) & ~(size_t)255;
    }
    void bind(void* base) const {
        for (int i = 0; i < n; i++) regions[i].set(regions[i].slot, static_cast<char*>(base) + regions[i].off);
    }
};

// ------------------------------------------------------------------ the engine
struct sc_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    scnn::NetDev net{};
    uint16_t* d_wb = nullptr;
    float* d_wf = nullptr;
    int n_cu = 256;    // compute units of the device
    int step_blocks_per_cu = 1;   // resident fused step workgroups per CU for this network (1 or 2)
    int ksplit = 64;   // split-K of value_head.ffn.0 (the search kernel's fused tail sums 32 or 64 partials)
    // scratch of the host-pointer calls and of self-play, grown on demand (engine_reserve: all for the same number of positions)
    DevBuf<int8_t> d_boards;
    DevBuf<int32_t> d_meta;
    DevBuf<uint16_t> d_lidx;
    DevBuf<int32_t> d_nlegal;
    DevBuf<float> d_prior;
    DevBuf<float> d_value;
    DevBuf<float> d_logp;
    DevBuf<float> d_dbg;
    // scratch arena of sc_encode_positions (Level-1 callers encode one position per call: no malloc/free per call)
    DevBuf<char> d_enc;
    // the one-slot handle sc_search keeps between calls (NNPlayer::bestmove calls it once per move: building and freeing ~35 device
    // buffers per call cost more than a short search) and the rollout its node pools are sized for
    struct sc_selfplay* search_sp = nullptr;
    int search_rollout_cap = 0;
    // d_hval / d_vpart grow by themselves (engine_reserve_hv): the device-pointer entry points (sc_forward_device,
    // sc_score_positions, sc_compare_engines) run enqueue_forward on the caller's tensors and need only these two, for one slice.
    // Their other scratch: the slice's values and log-probability rows (scoring only), and per-position results the caller did not
    // ask for but the summary needs.  dv_ev orders those calls (any stream) and the engine's stream after each other.
    DevBuf<scnn::bf16_t> d_hval;
    DevBuf<float> d_vpart;
    DevBuf<float> dv_value;
    DevBuf<float> dv_logp;
    DevBuf<float> dv_pp;
    hipEvent_t dv_ev = nullptr;
};

// growing a scratch buffer of the engine waits on the host for the engine's stream: its earlier work may use the old buffer
template <class T>
static int engine_grow(sc_engine* e, DevBuf<T>& b, size_t want) {
    return b.grow(want, [e] { return hipStreamSynchronize(e->stream); });
}
int engine_reserve(sc_engine* e, int n);      // all scratch of n positions (at least 64)
int engine_reserve_hv(sc_engine* e, int n);   // value-head features and split-K partials of n positions (enqueue_forward's scratch)

// the argument blocks of the tower and of value_head.ffn.0 for n positions of network e
scnn::TowerArgs tower_args(const sc_engine* e, int n, const int8_t* boards, const int32_t* meta, int meta_stride, const uint16_t* lidx,
                           const int32_t* nlegal, float* prior, float* logp, scnn::bf16_t* hval, float* dbg = nullptr, int dbg_stage = -1);
scnn::Fc1Args fc1_args(const sc_engine* e, int n, const scnn::bf16_t* hval, float* vpart);
// enqueue the three network kernels for n positions (device pointers)
void enqueue_forward(sc_engine* e, int n, const int8_t* boards, const int32_t* meta, int meta_stride, const uint16_t* lidx,
                     const int32_t* nlegal, float* prior, float* value, float* logp, float* dbg, int dbg_stage, hipStream_t s);

// ------------------------------------------------------------------ positions given as FEN (positions.hip)
// n validated records in device memory (fen_kernels.hip) and the host's copy of them, their status and the ep bit of Board.fen()
struct sc_positions {
    int device = 0;
    int n = 0;
    sc::Position* d_rec = nullptr;
    std::vector<sc::Position> rec;
    std::vector<int32_t> status;
    std::vector<int32_t> ep_legal;
};
// The bases of a call that takes them: checks the set's device and every index of idx[0..n) (host; < 0: no base) against the
// set -- a negative status is refused, and with for_search a status of 1 too -- and returns the records.  bases == nullptr or
// idx == nullptr: *d_rec = nullptr (no bases)
int positions_bases(const sc_positions* bases, const int32_t* idx, int n, int dev, bool for_search, const char* who, const sc::Position** d_rec);
// Board.fen() of a record
std::string position_fen(const sc::Position& p, bool ep_legal);
// text into a caller's buffer of cap bytes (cut to cap - 1 and terminated; cap == 0: nothing is written): the text's full length
int copy_text(const std::string& s, char* buf, int cap);

// ------------------------------------------------------------------ training tensors on the device (encode_steps.hip)
struct DevEncodeOut {
    int layout;
    void* boards;
    void* meta;
    float* dist;
    float* dist_legal;
    uint16_t* legal_idx;
    int32_t* n_legal;
    int32_t* status;
};
// the bases of a host call (rec == nullptr: none): the records on the device, the index of every game on the host (< 0: none)
struct HostBases { const sc::Position* rec; const int32_t* idx; };
// What an encode reads, one kind per call, and the games' optional bases.  ply_off is the call's in every kind.
struct EncodeSrc {
    enum Kind { CSR, RING, SAN, DEV } kind;
    const uint16_t *moves, *child_mv;     // CSR: host arrays as sc_encode_steps takes them.  DEV (sc_traces_encode_device): device arrays
    const uint32_t *child_n, *child_off;  // of a parsed set -- moves / child_off of the range's first ply on, child_off global into child_mv / child_n
    const int32_t* rows;      // RING (sc_selfplay_encode_traces): host, the ring row of each requested game; the moves and children
    const sc::SpParams* p;    // are read from the ring's rows on the device
    const uint64_t* tokens;   // SAN (sc_encode_san_device): host, one per ply; the moves are parsed on the device, every ply's
    uint16_t* moves_out;      // children are its legal moves with count 1 on the move played.  device [P] or null: the parsed moves
    HostBases bases;
    const int32_t* over;      // DEV: device [games], the codes the reader decided (0: the encoder's status stands)
    static EncodeSrc csr(const uint16_t* mv, const uint16_t* cmv, const uint32_t* cn, const uint32_t* coff, HostBases b) { return {CSR, mv, cmv, cn, coff, {}, {}, {}, {}, b}; }
    static EncodeSrc ring(const int32_t* rows, const sc::SpParams* p) { return {RING, {}, {}, {}, {}, rows, p, {}, {}, {}}; }
    static EncodeSrc san(const uint64_t* tokens, uint16_t* moves_out, HostBases b) { return {SAN, {}, {}, {}, {}, {}, {}, tokens, moves_out, b}; }
    static EncodeSrc dev(const uint16_t* mv, const uint16_t* cmv, const uint32_t* cn, const uint32_t* coff, const int32_t* over) {
        return {DEV, mv, cmv, cn, coff, {}, {}, {}, {}, HostBases{nullptr, nullptr}, over};
    }
};
// pointers the kernels of a call read or write must be device memory of `dev`; null entries are skipped
int check_device_ptrs(std::initializer_list<std::pair<const void*, const char*>> ptrs, int dev);
int check_device_outputs(const DevEncodeOut& o, int dev);
// the offsets of a batch of move lists (n + 1, host): monotonic, no list longer than 4000; with child_off also the children's
int check_traces(int n_games, const uint32_t* move_off, const uint32_t* child_off);
int encode_device_core(int dev, int n_games, const uint32_t* ply_off, const EncodeSrc& src, int apply_mirror, const DevEncodeOut& o,
                       hipStream_t st);

// ------------------------------------------------------------------ trace files read on the device (traces.hip)
// the packed arrays of n parsed files in device memory (trace_kernels.hip) and the host's copy of what is per file
struct sc_traces {
    int device = 0;
    int n = 0;
    uint16_t *d_moves = nullptr, *d_child_mv = nullptr, *d_opening = nullptr;
    uint32_t *d_child_off = nullptr, *d_child_n = nullptr;   // d_child_off [plies + 1]: global, the total behind the last ply
    int32_t* d_over = nullptr;   // [n]: 300000 + code of a refused file, 400000 with "opening" or "fen", else 0
    std::vector<int32_t> status, outcome, has_fen;
    std::vector<uint32_t> err_at, n_steps, n_children, n_opening;
    std::vector<uint32_t> move_off, child_base, open_off;   // [n + 1]: the prefix sums of the counts
    std::vector<char> fen;                                  // [n][128]
    // the ply offsets of the games from g0 on, rebased to 0, one array per g0 asked for: an encode uploads them asynchronously,
    // so they live as long as the handle
    mutable std::mutex mu;
    mutable std::map<int, std::vector<uint32_t>> range_off;
};
const uint32_t* traces_range_off(const sc_traces* t, int g0);

// text to a file, whole or appended
int write_text_file(const char* path, const std::string& text, bool append);

// ------------------------------------------------------------------ trace files written on the device (trace_write.hip)
// What a writer keeps between calls: its non-blocking stream, the events around its two passes, the device arena and text
// buffer and the pinned host buffer the text comes back to, all grown on demand.  sc_traces_format has one per call, a
// self-play handle keeps one (a hipFree per call would wait for the handle's step launches)
struct TraceWriter {
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    DevBuf<char> arena, text;
    char* pinned = nullptr;
    size_t pinned_cap = 0;
    TraceWriter() = default;
    TraceWriter(const TraceWriter&) = delete;
    TraceWriter& operator=(const TraceWriter&) = delete;
    ~TraceWriter() { release(); }
    void release();   // (the owner's device is current)
};

// ------------------------------------------------------- self-play (selfplay.hip, match_play.hip, selfplay_io.hip, report.hip, debug_calls.hip)
struct sc_selfplay {
    sc_engine* engine = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    sc_selfplay_config cfg{};
    sc::SpParams p{};
    std::vector<void*> allocs;
    int64_t sim_steps_enqueued = 0;
    // timing
    int timing_stride = 0;       // > 0: every n-th step runs as separate launches with the TOWER bracketed by an event pair
    int step_stride = 0;         // > 0: every n-th step is bracketed as a whole, in the handle's own launch form
    std::vector<hipEvent_t> ev;  // pairs
    int ev_next = 0;
    int64_t ev_recorded = 0;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    bool have_span = false;
    int64_t nn_launches = 0;
    bool pending_final = false;
    // match play (sc_selfplay_set_players): player of even / odd plies; with slot recycling (sc_selfplay_set_match, p.match_recycle)
    // players a / b, the evaluators of the launches t with (t / rollout) & 1 == 0 / 1
    bool match = false;
    sc_engine* player[2] = {nullptr, nullptr};
    uint64_t salt[2] = {0, 0};
    long long* d_match_sum = nullptr;   // sc_selfplay_match_tally: the tally summed over the slots [8]
    // an outside opponent (sc_selfplay_set_external, external_play.hip): 0, or 1 + colours -- the external_mode of the kernels.
    // ext_waiting: the slots that waited for the opponent at the last sc_selfplay_external_wait, -1 when a push or a search has
    // changed that since.  The device arrays of k_external_wait and k_push_moves, [n_slots] each, made by the first call that needs them
    int external = 0;
    int ext_waiting = -1;
    int32_t *d_ext_list = nullptr, *d_ext_count = nullptr, *d_ext_epl = nullptr, *d_push_slots = nullptr, *d_push_status = nullptr;
    sc::Position* d_ext_recs = nullptr;
    int4* d_ext_info = nullptr;
    uint16_t* d_push_moves = nullptr;
    // opening lines (sc_selfplay_set_openings): the lines' position records on the device, replayed once, and the host's copy of
    // the moves (sc_selfplay_get_opening, the trace JSON).  open_lines.n = 0: none
    sc::MatchLines open_lines{nullptr, nullptr, 0};
    std::vector<uint16_t> open_moves;
    std::vector<uint32_t> open_move_off;   // [n + 1]
    std::vector<std::string> open_fens;    // [n] or empty: the base of each line as Board.fen() prints it, "" for the start position
    scnn::bf16_t* d_hval = nullptr;  // value-head features of the current leaves [n_slots][16384], in the tower's accumulator order
    float* d_vpart = nullptr;        // split-K partials of value_head.ffn.0 [ksplit][n_slots][128]
    // streaming drain (sc_selfplay_poll): per trace-ring row, the game id last reported to the host (+1; 0 = none)
    std::vector<uint64_t> reported;
    std::vector<int> to_release;     // rows handed out by the previous poll (trace_hold)
    // sc_selfplay_encode_traces: recorded on the caller's stream behind the last encode that read ring rows; the next poll
    // waits for it before it releases rows
    hipEvent_t enc_ev = nullptr;
    bool enc_pending = false;
    // sc_selfplay_traces_json / sc_selfplay_write_traces_json: the handle's trace writer, created by the first such call
    TraceWriter* writer = nullptr;
    // sc_selfplay_report: the packed buffer the report kernel writes (report_types.hpp scrp::Packed), grown on demand, and the
    // event pair around the kernel, created by the first such call
    DevBuf<char> d_report;
    hipEvent_t report_ev[2] = {nullptr, nullptr};
    // sc_selfplay_advance (advance.hip): the call's arrays (slots, moves, status, kept, offsets) and the marks of k_advance, one
    // word per LIVE node of the listed slots (never node_cap x n_slots); made by the first such call, grown on demand
    DevBuf<char> d_adv;
    DevBuf<uint32_t> d_adv_marks;
    // search wave + tower in one launch (step_kernels.hip).  Chosen at creation: only with at most one game per compute
    // unit and a single group -- with more games than CUs the separate search launch runs all of them at once while the
    // fused workgroups (83 KB of LDS: one per CU) would take turns, and with several interleaved groups one group's search
    // launch is what hides under another group's tower (measured: 512 games 3.48 M vs 3.02 M simulations/s at fp8, two
    // groups of 256 2.65 M vs 2.38 M at bf16, in favour of the separate launches)
    bool fused = false;
    bool fc1_in_step = false;        // ... and value_head.ffn.0 runs inside that launch too (one launch per simulation step)
    uint32_t* d_fc1_ctr = nullptr;   // its arrival counters, one per 64-position block, 128 B apart (monotonic)
    uint32_t fc1_launches = 0;       // step launches that counted on them so far
    uint32_t fc1_target_skew = 0;    // test aid (sc_selfplay_debug_break_handoff): arrivals that will never come
    // An internal hand-off of a step launch timed out (error_flags & (16 | 32)): tiles were computed from stale rows, the
    // values backed up since are wrong.  Latched when the host first sees the flag; from then on the handle refuses work.
    bool poisoned = false;
};

// a device buffer that lives as long as the handle.  The zero-fill runs on the handle's stream, ahead of every launch on it
template <class T>
static int sp_alloc(sc_selfplay* sp, T** ptr, size_t n, bool zero = true) {
    HIPOK(dalloc(ptr, n));
    sp->allocs.push_back(*ptr);
    if (zero) HIPOK(hipMemsetAsync(*ptr, 0, std::max<size_t>(n, 1) * sizeof(T), sp->stream));
    return 0;
}
// The weights of the end-of-ply move choice, w[n] = powf((float)n, 1.0f / temperature) for n = 0..n_max, by the host libm
// (selfplay.hip): the table of a handle and of sc_debug_choose_child
std::vector<float> choice_weights(float temperature, int n_max);

int sp_refuse(const sc_selfplay* sp);   // the error of a poisoned handle
// A row that sc_selfplay_poll has reported and holds (trace_hold) is final, and no kernel writes it until the next poll releases it
bool row_held(const sc_selfplay* sp, int row, uint64_t want_id);
// the ring row may belong to an earlier game (the wanted one has not started), to a later one (overwritten) or be released
enum RowState { ROW_READY, ROW_NOT_FINISHED, ROW_GONE };
RowState row_state(const sc_selfplay* sp, int row, uint64_t want_id, const sc::TraceHdr& h);
// The opening of a host read or write: set the device, complete the last enqueued simulation (expand / backward / ply transition:
// host reads see a fully backed-up state), wait for the stream; with `latch` also look at the device's error word, and refuse a
// poisoned handle
int sp_quiesce(sc_selfplay* sp, bool latch);
// n simulation steps in the handle's launch form (the body of sc_selfplay_enqueue_sims, which refuses an external handle), and the
// first half of the launch the next step would start with, where one is pending (selfplay.hip)
int sp_enqueue_steps(sc_selfplay* sp, int n);
void sp_flush(sc_selfplay* sp);
// the opening line of handle-local game `game` (sc_selfplay_set_openings): its length, *moves = its first move; 0 without lines
int sp_opening(const sc_selfplay* sp, int game, const uint16_t** moves);
// the base of that line (sc_selfplay_set_openings_from) as FEN text, or null for a line from the start position
const char* sp_opening_fen(const sc_selfplay* sp, int game);

#pragma GCC visibility pop
