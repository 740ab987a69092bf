// engine.hip -- host side of libsc_engine.so: the C ABI of include/sc_engine.h over the HIP kernels.  This unit: the engine and
// its host-pointer calls, the helpers of host_common.hpp; training tensors are in encode_steps.hip, the calls on device tensors in
// device_calls.hip, self-play in selfplay.hip, match_play.hip, selfplay_io.hip and debug_calls.hip.
//
// Replaces, behind the reference's own interfaces: backend construction + Game::predict
// (src/main.rs:83-128, src/backends/torch.rs:89-146), the rules/encoder calls into python-chess
// (src/chess.rs:665-877) and the per-game self-play loop (src/main.rs:155-238) -- the latter for
// many concurrent games per GPU.  All compute runs on the GPU; there is no CPU fallback: every
// entry point fails with an error code if HIP or the device is unavailable.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "host_common.hpp"
#include "trace_json.hpp"
#include "weights.hpp"

// The C ABI's structs are bound field by field from Rust (integration/hip.rs), ctypes (scamd/binding.py) and C: their layout
// is part of the interface.  A new field goes at the END, together with the bindings (tests/test_abi.py compares all three).
#define SC_LAYOUT(T, size) static_assert(sizeof(T) == (size), #T ": size changed -- update integration/hip.rs and scamd/binding.py")
#define SC_FIELD(T, f, off) static_assert(offsetof(T, f) == (off), #T "." #f ": offset changed")
SC_LAYOUT(sc_net_config, 24);
SC_FIELD(sc_net_config, n_res_blocks, 0); SC_FIELD(sc_net_config, channels, 4); SC_FIELD(sc_net_config, seed, 8);
SC_FIELD(sc_net_config, precision, 16); SC_FIELD(sc_net_config, reserved, 20);
SC_LAYOUT(sc_selfplay_config, 88);
SC_FIELD(sc_selfplay_config, n_slots, 0); SC_FIELD(sc_selfplay_config, n_games, 4); SC_FIELD(sc_selfplay_config, rollout_num, 8);
SC_FIELD(sc_selfplay_config, num_steps, 12); SC_FIELD(sc_selfplay_config, cpuct, 16); SC_FIELD(sc_selfplay_config, temperature, 20);
SC_FIELD(sc_selfplay_config, temperature_switch, 24); SC_FIELD(sc_selfplay_config, epsilon, 28); SC_FIELD(sc_selfplay_config, with_noise, 32);
SC_FIELD(sc_selfplay_config, outcome_gate, 36); SC_FIELD(sc_selfplay_config, evaluator, 40); SC_FIELD(sc_selfplay_config, external_noise, 44);
SC_FIELD(sc_selfplay_config, seed, 48); SC_FIELD(sc_selfplay_config, first_game_id, 56); SC_FIELD(sc_selfplay_config, trace_capacity, 64);
SC_FIELD(sc_selfplay_config, own_stream, 68); SC_FIELD(sc_selfplay_config, tie_random, 72); SC_FIELD(sc_selfplay_config, trace_hold, 76);
SC_FIELD(sc_selfplay_config, rollout_factor, 80);
SC_LAYOUT(sc_selfplay_stats, 32);
SC_FIELD(sc_selfplay_stats, sims_done, 0); SC_FIELD(sc_selfplay_stats, nn_evals, 8); SC_FIELD(sc_selfplay_stats, games_finished, 16);
SC_FIELD(sc_selfplay_stats, games_active, 20); SC_FIELD(sc_selfplay_stats, error_flags, 24); SC_FIELD(sc_selfplay_stats, plies_done, 28);
SC_LAYOUT(sc_trace_info, 32);
SC_FIELD(sc_trace_info, n_steps, 0); SC_FIELD(sc_trace_info, n_children_total, 4); SC_FIELD(sc_trace_info, has_outcome, 8);
SC_FIELD(sc_trace_info, termination, 12); SC_FIELD(sc_trace_info, winner, 16); SC_FIELD(sc_trace_info, game_id, 24);
#undef SC_LAYOUT
#undef SC_FIELD

thread_local std::string g_err;
static thread_local std::string g_warn;
int write_text_file(const char* path, const std::string& text, bool append) {
    FILE* f = fopen(path, append ? "ab" : "wb");
    if (!f) return fail(std::string("cannot open ") + path);
    const size_t w = fwrite(text.data(), 1, text.size(), f);
    fclose(f);
    return w == text.size() ? 0 : fail("short write");
}

int fail(const std::string& m, int code) {
    g_err = m;
    return code;
}

int use_device(const sc_engine* e, int device_id) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail("no HIP device available: libsc_engine has no CPU fallback", -3);
    const int dev = e ? e->device : device_id;
    if (dev < 0 || dev >= ndev) return fail("device_id out of range");
    HIPOK(hipSetDevice(dev));
    return 0;
}

int engine_reserve_hv(sc_engine* e, int n) {
    TRY(engine_grow(e, e->d_hval, (size_t)n * 64 * 256));
    return engine_grow(e, e->d_vpart, (size_t)e->ksplit * n * 128);
}
int engine_reserve(sc_engine* e, int n) {
    const size_t cap = (size_t)std::max(n, 64);
    TRY(engine_grow(e, e->d_boards, cap * 7168));
    TRY(engine_grow(e, e->d_meta, cap * 8));
    TRY(engine_grow(e, e->d_lidx, cap * 224));
    TRY(engine_grow(e, e->d_nlegal, cap));
    TRY(engine_grow(e, e->d_prior, cap * 224));
    TRY(engine_grow(e, e->d_value, cap));
    TRY(engine_grow(e, e->d_logp, cap * 4672));
    TRY(engine_grow(e, e->d_dbg, cap * 64 * 256));
    return engine_reserve_hv(e, (int)cap);
}

scnn::TowerArgs tower_args(const sc_engine* e, int n, const int8_t* boards, const int32_t* meta, int meta_stride, const uint16_t* lidx,
                           const int32_t* nlegal, float* prior, float* logp, scnn::bf16_t* hval, float* dbg, int dbg_stage) {
    scnn::TowerArgs t{};
    t.net = e->net;
    t.n_pos = n;
    t.boards = boards;
    t.meta = meta;
    t.meta_stride = meta_stride;
    t.legal_idx = lidx;
    t.n_legal = nlegal;
    t.prior = (lidx && nlegal) ? prior : nullptr;
    t.logp = logp;
    t.hval = hval;
    t.dbg = dbg;
    t.dbg_stage = dbg ? dbg_stage : -1;
    return t;
}
scnn::Fc1Args fc1_args(const sc_engine* e, int n, const scnn::bf16_t* hval, float* vpart) {
    scnn::Fc1Args f{};
    f.net = e->net;
    f.n_pos = n;
    f.ksplit = e->ksplit;
    f.hval = hval;
    f.vpart = vpart;
    return f;
}

void enqueue_forward(sc_engine* e, int n, const int8_t* boards, const int32_t* meta, int meta_stride, const uint16_t* lidx,
                     const int32_t* nlegal, float* prior, float* value, float* logp, float* dbg, int dbg_stage, hipStream_t s) {
    scl::tower(tower_args(e, n, boards, meta, meta_stride, lidx, nlegal, prior, logp, e->d_hval.p, dbg, dbg_stage), s);
    scl::value_fc1(fc1_args(e, n, e->d_hval.p, e->d_vpart.p), s);
    scnn::VfinArgs v{};
    v.net = e->net;
    v.n_pos = n;
    v.ksplit = e->ksplit;
    v.vpart = e->d_vpart.p;
    v.meta = meta;
    v.meta_stride = meta_stride;
    v.value = value;
    scl::value_finish(v, s);
}

extern "C" {

const char* sc_last_error(void) { return g_err.c_str(); }

int sc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// Kernel arguments in device memory: with the default (host-coherent) placement every launch starts with a PCIe round
// trip for its argument block -- three launches per simulation step, +6 % simulations/s measured.  The HIP runtime reads the
// switch when it initialises, so it is set when this library is loaded (no effect if the host application has already
// initialised HIP: export HIP_FORCE_DEV_KERNARG=1 there).  An explicit setting of the host wins.
// SC_ENGINE_KEEP_ENV=1 disables the hook.  sc_runtime_flags() reports what happened (include/sc_engine.h).
namespace {
struct RuntimeEnv {
    int flags = 0;
    RuntimeEnv() {
        const char* keep = getenv("SC_ENGINE_KEEP_ENV");
        if (keep && keep[0] == '1') {
            flags |= 4;
        } else if (!getenv("HIP_FORCE_DEV_KERNARG")) {
            setenv("HIP_FORCE_DEV_KERNARG", "1", 0);
            flags |= 2;
        }
    }
} g_runtime_env;
}  // namespace

int sc_runtime_flags(void) {
    const char* v = getenv("HIP_FORCE_DEV_KERNARG");
    const int on = (v && v[0] == '1' && v[1] == 0) ? 1 : 0;
    return on | (on ? (g_runtime_env.flags & 2) : 0) | (g_runtime_env.flags & 4);
}
const char* sc_last_warning(void) { return g_warn.c_str(); }

int sc_engine_create(const sc_net_config* cfg, const char* weights_path, int device_id, sc_engine** out) {
    if (!cfg || !out) return fail("null argument");
    *out = nullptr;
    TRY(use_device(nullptr, device_id));
    scw::HostWeights hw;
    if (weights_path) {
        std::string err = scw::load_scw(weights_path, hw);
        if (!err.empty()) return fail(err);
    } else {
        if (cfg->channels != 128 && cfg->channels != 256) return fail("channels must be 128 or 256");
        if (cfg->n_res_blocks < 0 || cfg->n_res_blocks > 80) return fail("n_res_blocks out of range");
        hw = scw::init_prng(cfg->n_res_blocks, cfg->channels, cfg->seed);
    }
    if (cfg->precision != SC_PREC_BF16 && cfg->precision != SC_PREC_FP8) return fail("unknown precision");
    if (cfg->precision == SC_PREC_FP8) hw.fp8 = true;   // (an SCW2 fp8 blob sets it by itself)
    // Both trunk widths run the channel-major 32x32x16 tower.
    scw::Packed pk = scw::pack(hw);
    sc_engine* e = new sc_engine();
    e->device = device_id;
    // every failure from here on goes through sc_engine_destroy (stream, weight blobs)
    auto bail = [&](hipError_t err, const char* what) {
        std::string m = std::string(what) + ": " + hipGetErrorString(err);
        sc_engine_destroy(e);
        return fail(m, -2);
    };
    const char* ierr = scl::nn_init();
    if (!ierr) ierr = scl::step_init();
    if (ierr) {
        sc_engine_destroy(e);
        return fail(std::string("kernel attribute setup failed: ") + ierr);
    }
    hipError_t he;
    if ((he = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking)) != hipSuccess) return bail(he, "hipStreamCreate");
    if ((he = dalloc(&e->d_wb, pk.wb.size())) != hipSuccess) return bail(he, "hipMalloc(weights)");
    if ((he = dalloc(&e->d_wf, pk.wf.size())) != hipSuccess) return bail(he, "hipMalloc(parameters)");
    if ((he = hipMemcpy(e->d_wb, pk.wb.data(), pk.wb.size() * 2, hipMemcpyHostToDevice)) != hipSuccess) return bail(he, "hipMemcpy(weights)");
    if ((he = hipMemcpy(e->d_wf, pk.wf.data(), pk.wf.size() * 4, hipMemcpyHostToDevice)) != hipSuccess) return bail(he, "hipMemcpy(parameters)");
    {
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && ncu > 0) e->n_cu = ncu;
    }
    static_cast<scnn::NetLayout&>(e->net) = pk.lay;
    e->step_blocks_per_cu = std::min(2, scl::step_blocks_per_cu(pk.lay));
    e->net.wb = e->d_wb;
    e->net.wf = e->d_wf;
    const int rf = sc_runtime_flags();
    g_warn.clear();
    if (!(rf & 1))
        g_warn = "HIP_FORCE_DEV_KERNARG=1 is not set: kernel arguments travel through host-coherent memory (about -6 % simulations/s)";
    else if (rf & 2)
        g_warn = "HIP_FORCE_DEV_KERNARG=1 was set by libsc_engine's load hook: it has no effect if the host initialised HIP before "
                 "loading the library (export it in the host's environment instead)";
    *out = e;
    return 0;
}

void sc_engine_destroy(sc_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->search_sp) {
        sc_selfplay_destroy(e->search_sp);
        e->search_sp = nullptr;
    }
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    dfree({e->d_boards.p, e->d_meta.p, e->d_lidx.p, e->d_nlegal.p, e->d_prior.p, e->d_value.p, e->d_logp.p, e->d_dbg.p, e->d_enc.p});
    dfree({e->d_hval.p, e->d_vpart.p, e->dv_value.p, e->dv_logp.p, e->dv_pp.p, e->d_wb, e->d_wf});
    if (e->dv_ev) (void)hipEventDestroy(e->dv_ev);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

int sc_engine_max_batch(const sc_engine*) { return 65536; }
int sc_engine_precision(const sc_engine* e) { return e && e->net.fp8 ? SC_PREC_FP8 : SC_PREC_BF16; }
int sc_engine_synchronize(sc_engine* e) {
    if (!e) return fail("null engine");
    HIPOK(hipSetDevice(e->device));
    HIPOK(hipStreamSynchronize(e->stream));
    return 0;
}

static int forward_host(sc_engine* e, int n, const int8_t* boards, const int32_t* meta, const uint16_t* lidx_rows,
                        const int32_t* nlegal, float* prior_rows, float* value, float* logp, float* dbg, int dbg_stage) {
    if (!e || !boards || !meta || n < 0) return fail("bad argument");
    if (n == 0) return 0;
    HIPOK(hipSetDevice(e->device));
    TRY(engine_reserve(e, n));
    hipStream_t s = e->stream;
    HIPOK(hipMemcpyAsync(e->d_boards.p, boards, (size_t)n * 7168, hipMemcpyHostToDevice, s));
    {
        std::vector<int32_t> m8((size_t)n * 8, 0);
        for (int i = 0; i < n; i++)
            for (int k = 0; k < 7; k++) m8[(size_t)i * 8 + k] = meta[(size_t)i * 7 + k];
        HIPOK(hipMemcpy(e->d_meta.p, m8.data(), m8.size() * 4, hipMemcpyHostToDevice));
    }
    if (lidx_rows) {
        HIPOK(hipMemcpyAsync(e->d_lidx.p, lidx_rows, (size_t)n * 224 * 2, hipMemcpyHostToDevice, s));
        HIPOK(hipMemcpyAsync(e->d_nlegal.p, nlegal, (size_t)n * 4, hipMemcpyHostToDevice, s));
    }
    enqueue_forward(e, n, e->d_boards.p, e->d_meta.p, 8, lidx_rows ? e->d_lidx.p : nullptr, lidx_rows ? e->d_nlegal.p : nullptr,
                    e->d_prior.p, e->d_value.p, logp ? e->d_logp.p : nullptr, dbg ? e->d_dbg.p : nullptr, dbg_stage, s);
    HIPOK(hipGetLastError());
    if (value) HIPOK(hipMemcpyAsync(value, e->d_value.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (logp) HIPOK(hipMemcpyAsync(logp, e->d_logp.p, (size_t)n * 4672 * 4, hipMemcpyDeviceToHost, s));
    if (prior_rows) HIPOK(hipMemcpyAsync(prior_rows, e->d_prior.p, (size_t)n * 224 * 4, hipMemcpyDeviceToHost, s));
    if (dbg) HIPOK(hipMemcpyAsync(dbg, e->d_dbg.p, (size_t)n * 64 * e->net.C * 4, hipMemcpyDeviceToHost, s));
    HIPOK(hipStreamSynchronize(s));
    return 0;
}

int sc_forward_batch(sc_engine* e, int n, const int8_t* boards, const int32_t* meta, float* logp, float* value) {
    return forward_host(e, n, boards, meta, nullptr, nullptr, nullptr, value, logp, nullptr, -1);
}

/* debugging aid for tests: residual stream after `stage` (0: after the stem, b: after the b-th residual block, 1-based, 1000: the
 * latent): out[n][64][C] */
int sc_forward_debug(sc_engine* e, int n, const int8_t* boards, const int32_t* meta, int stage, float* out) {
    return forward_host(e, n, boards, meta, nullptr, nullptr, nullptr, nullptr, nullptr, out, stage);
}

int sc_predict_batch(sc_engine* e, int n, const int8_t* boards, const int32_t* meta, const uint16_t* legal_idx,
                     const uint32_t* legal_off, float* priors, float* value) {
    if (!legal_idx || !legal_off || !priors) return fail("bad argument");
    std::vector<uint16_t> rows((size_t)n * 224, 0);
    std::vector<int32_t> nl((size_t)n);
    for (int i = 0; i < n; i++) {
        uint32_t a = legal_off[i], b = legal_off[i + 1];
        if (b < a || b - a > 218) return fail("legal_off: more than 218 moves for one position");
        nl[(size_t)i] = (int32_t)(b - a);
        for (uint32_t k = a; k < b; k++) {
            if (legal_idx[k] >= 4672) return fail("legal_idx out of range");
            rows[(size_t)i * 224 + (k - a)] = legal_idx[k];
        }
    }
    std::vector<float> pr((size_t)n * 224);
    int rc = forward_host(e, n, boards, meta, rows.data(), nl.data(), pr.data(), value, nullptr, nullptr, -1);
    if (rc) return rc;
    for (int i = 0; i < n; i++)
        for (int k = 0; k < nl[(size_t)i]; k++) priors[legal_off[i] + (uint32_t)k] = pr[(size_t)i * 224 + k];
    return 0;
}

/* Game::predict with argmax = true: post_process_distr's first branch (src/chess.rs:880-889) -- a one-hot vector at the
 * LAST maximal prior of each position (Iterator::max_by).  The maximum is taken over the renormalised priors: the
 * reference takes it over exp(logp[idx]) before the division, which orders the moves the same way except where two
 * different values round to the same quotient. */
int sc_predict_batch_argmax(sc_engine* e, int n, const int8_t* boards, const int32_t* meta, const uint16_t* legal_idx,
                            const uint32_t* legal_off, float* priors, float* value) {
    int rc = sc_predict_batch(e, n, boards, meta, legal_idx, legal_off, priors, value);
    if (rc) return rc;
    for (int i = 0; i < n; i++) {
        const uint32_t a = legal_off[i], b = legal_off[i + 1];
        if (b == a) continue;
        uint32_t best = a;
        for (uint32_t k = a + 1; k < b; k++)
            if (!(priors[k] < priors[best])) best = k;   // >= : the last maximum; a NaN prior wins like partial_cmp().unwrap() would panic
        for (uint32_t k = a; k < b; k++) priors[k] = k == best ? 1.0f : 0.0f;
    }
    return 0;
}

int sc_encode_positions(sc_engine* e, int device_id, int n, const uint16_t* moves, const uint32_t* move_off, int8_t* boards,
                        int32_t* meta, uint16_t* legal_moves, uint16_t* legal_idx, int32_t* n_legal, int32_t* outcome) {
    return sc_encode_positions_from(e, device_id, n, nullptr, nullptr, moves, move_off, boards, meta, legal_moves, legal_idx, n_legal, outcome);
}

// ... from a base per position (a set of validated records, positions.hip); without bases the call above
int sc_encode_positions_from(sc_engine* e, int device_id, int n, const sc_positions* bases, const int32_t* base_idx, const uint16_t* moves,
                             const uint32_t* move_off, int8_t* boards, int32_t* meta, uint16_t* legal_moves, uint16_t* legal_idx,
                             int32_t* n_legal, int32_t* outcome) {
    if (n < 0 || !move_off) return fail("bad argument");
    if (n == 0) return 0;
    TRY(use_device(e, device_id));
    const sc::Position* d_bases = nullptr;
    TRY(positions_bases(bases, base_idx, n, e ? e->device : device_id, false, "sc_encode_positions_from", &d_bases));
    TRY(check_traces(n, move_off, nullptr));
    uint32_t total = move_off[n], maxlen = 0;
    for (int i = 0; i < n; i++) maxlen = std::max(maxlen, move_off[i + 1] - move_off[i]);
    int hist_cap = (int)maxlen + 2;
    // one arena for all device buffers of the call; with an engine it persists (grown on demand) and the copies run on
    // the engine's stream behind a single synchronisation
    uint16_t *d_moves, *d_lm, *d_li;
    uint32_t* d_off;
    sc::Position* d_hist;
    int8_t* d_boards;
    int32_t *d_meta, *d_nl, *d_out, *d_bidx;
    ArenaLayout L;
    L.add(&d_moves, (size_t)total + 1);
    L.add(&d_off, (size_t)n + 1);
    L.add(&d_bidx, (size_t)n, d_bases != nullptr);
    L.add(&d_hist, (size_t)n * hist_cap);
    L.add(&d_boards, (size_t)n * 7168);
    L.add(&d_meta, (size_t)n * 7);
    L.add(&d_nl, (size_t)n);
    L.add(&d_out, (size_t)n * 4);
    L.add(&d_lm, (size_t)n * 224);
    L.add(&d_li, (size_t)n * 224);
    ScopedDev<char> local;   // without an engine: this call's own
    hipStream_t st = e ? e->stream : nullptr;
    if (e) TRY(engine_grow(e, e->d_enc, L.bytes));
    else HIPOK(local.alloc(L.bytes));
    L.bind(e ? e->d_enc.p : local.p);
    if (total) HIPOK(hipMemcpyAsync(d_moves, moves, (size_t)total * 2, hipMemcpyHostToDevice, st));
    HIPOK(hipMemcpyAsync(d_off, move_off, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, st));
    HIPOK(hipMemsetAsync(d_lm, 0, (size_t)n * 448, st));   // rows are zero past n_legal (each region is padded to 256 B:
    HIPOK(hipMemsetAsync(d_li, 0, (size_t)n * 448, st));   // the two tables are not adjacent in general)
    if (d_bases) HIPOK(hipMemcpyAsync(d_bidx, base_idx, (size_t)n * 4, hipMemcpyHostToDevice, st));
    scl::encode_positions({n, d_moves, d_off, d_hist, hist_cap, {d_bases, d_bidx}}, {d_boards, d_meta, d_lm, d_li, d_nl}, d_out, st);
    HIPOK(hipGetLastError());
    if (boards) HIPOK(hipMemcpyAsync(boards, d_boards, (size_t)n * 7168, hipMemcpyDeviceToHost, st));
    if (meta) HIPOK(hipMemcpyAsync(meta, d_meta, (size_t)n * 7 * 4, hipMemcpyDeviceToHost, st));
    if (legal_moves) HIPOK(hipMemcpyAsync(legal_moves, d_lm, (size_t)n * 224 * 2, hipMemcpyDeviceToHost, st));
    if (legal_idx) HIPOK(hipMemcpyAsync(legal_idx, d_li, (size_t)n * 224 * 2, hipMemcpyDeviceToHost, st));
    if (n_legal) HIPOK(hipMemcpyAsync(n_legal, d_nl, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (outcome) HIPOK(hipMemcpyAsync(outcome, d_out, (size_t)n * 16, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    return 0;
}


int sc_trace_write_json(const char* path, const sc_trace_info* info, const uint16_t* step_move, const float* step_q,
                        const int32_t* child_off, const uint16_t* child_move, const int32_t* child_n, const float* child_q,
                        const float* child_uct) {
    if (!path || !info) return fail("bad argument");
    return write_text_file(path, sctrace::trace_to_json(info->n_steps, info->has_outcome, info->termination, info->winner, step_move, step_q,
                                                        child_off, child_move, child_n, child_q, child_uct), false);
}

int sc_move_uci(uint16_t move, char* buf8) { return sctrace::move_uci(move, buf8); }

// libsmartchess.chess_encode_move(turn, move) (reference src/lib.rs:37-44): the 4672-wide action index of a move for
// the side to move (Black's moves are rotated first); -1 if the move has no index.  Pure integer host function.
int sc_move_index(uint16_t move, int white_to_move) { return sc::move_index((sc::move_t)move, white_to_move ? sc::WHITE : sc::BLACK); }

}  // extern "C"
