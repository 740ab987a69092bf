// selfplay.hip -- host side of libsc_engine.so: the self-play handle and its stepping (stream grant, create, enqueue, statistics, timing).
//
// Step launches that compute value_head.ffn.0 inside the launch (sp->fc1_in_step) make workgroups wait for other workgroups
// of the same launch.  Two such launches running side by side on one device (two streams) could each hold compute units the
// other's late workgroups need: on one device the form is therefore granted to the handles of ONE stream at a time (the first
// to ask; an engine's handles share its stream and run one after the other); any other handle uses the two-launch form.
// (Two PROCESSES sharing a GPU are not covered: the waits are bounded -- error flag 32 -- but one self-play process per GPU
// is the deployment this library is written for.)
#include <math.h>

#include <map>
#include <memory>
#include <mutex>

#include "host_common.hpp"

// One record per device.  A device on which an in-launch hand-off has timed out once (the workgroups of a launch were not all
// resident: someone else is using the GPU) is not trusted with that form again by this process: handles created afterwards use the
// two-launch form, whose launches do not wait for each other.
struct Fc1Grant {
    hipStream_t stream = nullptr;
    int live = 0;   // handles that hold the grant
    bool failed = false;
};
static std::mutex g_fc1_mu;
static std::map<int, Fc1Grant> g_fc1;
static bool fc1_stream_acquire(int device, hipStream_t s) {
    std::lock_guard<std::mutex> lk(g_fc1_mu);
    Fc1Grant& g = g_fc1[device];
    if (g.failed || (g.live > 0 && g.stream != s)) return false;
    g.stream = s;
    g.live++;
    return true;
}
static void fc1_stream_release(int device) {
    std::lock_guard<std::mutex> lk(g_fc1_mu);
    Fc1Grant& g = g_fc1[device];
    if (g.live > 0) g.live--;
}

int sp_refuse(const sc_selfplay*) {
    return fail("an internal hand-off of this handle's step launches timed out (error_flags & 48): its trees and traces are "
                "invalid; destroy the handle -- a new handle on this device uses the two-launch step", SC_ERR_HANDOFF);
}
// called with the stream idle: looks at the device's error word
static int sp_latch(sc_selfplay* sp) {
    if (sp->poisoned) return 0;
    int32_t err = 0;
    HIPOK(hipMemcpy(&err, reinterpret_cast<const char*>(sp->p.cnt) + offsetof(sc::Counters, err), 4, hipMemcpyDeviceToHost));
    if (err & (sc::ERR_HELPER_TIMEOUT | sc::ERR_HANDOFF_TIMEOUT)) {
        sp->poisoned = true;
        if (err & sc::ERR_HANDOFF_TIMEOUT) {
            std::lock_guard<std::mutex> lk(g_fc1_mu);
            g_fc1[sp->device].failed = true;
        }
    }
    return 0;
}

// the value tail's weights are those of network e
static void set_value_tail(sc::SpParams& q, const sc_engine* e) {
    q.vf_w = e->d_wf;
    q.vf_fc1b = (uint32_t)e->net.f_fc1b;
    q.vf_fc1m = (uint32_t)e->net.f_fc1m;
    q.vf_fc2w = (uint32_t)e->net.f_fc2w;
    q.vf_fc2b = (uint32_t)e->net.f_fc2b;
}
// match play: the value tail of simulation step t uses the weights of the player that evaluated step t
static void match_tail_params(const sc_selfplay* sp, sc::SpParams& q, int64_t t) {
    if (!sp->match || sp->p.evaluator != SC_EVAL_NET || t < 0) return;
    set_value_tail(q, sp->player[(t / sp->p.rollout) & 1]);
}
// Match play with slot recycling.  The search launches never start a game (total_games = 0: a slot whose game ends goes idle);
// games start at the ply boundaries, t % rollout == 0, between the two halves of launch t: after the expansions that end the
// ply, k_match_boundary counts the games that ended and starts those whose White is the player of launch t, (t / rollout) & 1.
// (An external handle, sc_selfplay_set_external, has its own boundary kernels and runs them itself: external_play.hip.)
static void match_search_params(const sc_selfplay* sp, sc::SpParams& q) {
    if (sp->p.match_recycle || sp->external) q.total_games = 0;
}
static void match_boundary(const sc_selfplay* sp, int64_t t) {
    sc::SpParams q = sp->p;
    q.match_side = (uint8_t)((t / q.rollout) & 1);
    scl::match_boundary(q, sp->open_lines, sp->stream);
}
// complete the last enqueued simulation; a following enqueue would have done the same work in its first launch
void sp_flush(sc_selfplay* sp) {
    if (sp->pending_final) {
        sc::SpParams q = sp->p;
        match_tail_params(sp, q, sp->sim_steps_enqueued - 1);
        match_search_params(sp, q);
        scl::mcts(q, 1, 0, sp->stream);   // the first half of the launch that the next enqueue starts with
        if (sp->p.match_recycle && sp->sim_steps_enqueued % sp->p.rollout == 0) match_boundary(sp, sp->sim_steps_enqueued);
        sp->pending_final = false;
    }
}
int sp_quiesce(sc_selfplay* sp, bool latch) {
    HIPOK(hipSetDevice(sp->device));
    sp_flush(sp);
    HIPOK(hipStreamSynchronize(sp->stream));
    if (!latch) return 0;
    TRY(sp_latch(sp));
    return sp->poisoned ? sp_refuse(sp) : 0;
}

// The weights of the end-of-ply move choice (mcts::step, src/mcts.rs:313-315): w[n] = powf((float)n, 1.0f / temperature) for
// n = 0..n_max, computed HERE, by the host libm -- the function the reference's f32::powf is.  The kernels read the table
// instead of calling the device's powf, whose results differ from the host's in the last bit, because the sampled
// index has to be the reference's bit for bit.
std::vector<float> choice_weights(float temperature, int n_max) {
    const float power = 1.0f / temperature;
    std::vector<float> w((size_t)n_max + 1);
    for (int n = 0; n <= n_max; n++) w[(size_t)n] = powf((float)n, power);
    return w;
}

// ------------------------------------------------------------------ sc_selfplay_create, in four steps
static int create_check(const sc_engine* e, const sc_selfplay_config* cfg) {
    if (cfg->evaluator == SC_EVAL_NET && !e) return fail("SC_EVAL_NET needs an engine");
    if (cfg->n_slots <= 0 || cfg->n_games <= 0 || cfg->rollout_num < 1 || cfg->num_steps < 1 || cfg->num_steps > 4000)
        return fail("bad self-play configuration");
    if (cfg->rollout_num > 60000) return fail("rollout_num too large");
    if (cfg->evaluator < SC_EVAL_NET || cfg->evaluator > SC_EVAL_SYNTH_UNIFORM) return fail("unknown evaluator");
    if (cfg->rollout_factor < 0.f || (cfg->rollout_factor > 0.f && cfg->rollout_num != 300))
        return fail("rollout_factor needs rollout_num = 300 (the cap of min(300, n_legal * factor), src/main.rs:176)");
    return 0;
}

static void create_params(sc::SpParams& p, const sc_selfplay_config* cfg) {
    p.n_slots = cfg->n_slots;
    p.rollout = cfg->rollout_num;
    p.num_steps = cfg->num_steps;
    p.temp_switch = cfg->temperature_switch;
    p.with_noise = cfg->with_noise;
    p.outcome_gate = cfg->outcome_gate;
    p.evaluator = cfg->evaluator;
    p.external_noise = cfg->external_noise;
    p.tie_random = cfg->tie_random;
    p.trace_hold = cfg->trace_hold ? 1 : 0;
    p.rollout_factor = cfg->rollout_factor;
    p.synth_salt = 0;
    p.cpuct = cfg->cpuct;
    p.temperature = cfg->temperature;
    p.epsilon = cfg->epsilon;
    p.seed = cfg->seed;
    p.first_game_id = cfg->first_game_id;
    p.node_cap = 1 + cfg->rollout_num * 218;         // worst case: every expansion adds 218 children
    p.max_depth = std::min(cfg->rollout_num + 2, 1024);  // the path is tracked in LDS (search_select.hpp DEPTH_LDS)
    p.hist_cap = cfg->num_steps + 2 + 600;           // room for sc_selfplay_set_position prefixes
    p.tpos_cap = cfg->rollout_num + 2;
    p.trace_cap = cfg->trace_capacity > 0 ? std::min(cfg->n_games, std::max(cfg->trace_capacity, 2 * cfg->n_slots)) : cfg->n_games;
    p.total_games = cfg->n_games;
}

// every buffer of the handle (sp->stream exists: the zero-fills run on it) and the table of the move choice
static int create_alloc(sc_selfplay* sp) {
    sc::SpParams& p = sp->p;
    const size_t G = (size_t)p.n_slots, NC = (size_t)p.node_cap;
    TRY(sp_alloc(sp, &p.ctl, G));
    TRY(sp_alloc(sp, &p.hist, G * p.hist_cap, false));
    TRY(sp_alloc(sp, &p.tpos, G * p.tpos_cap, false));
    TRY(sp_alloc(sp, &p.path, G * p.max_depth));
    TRY(sp_alloc(sp, &p.N, G * NC, false));
    TRY(sp_alloc(sp, &p.W, G * NC, false));
    TRY(sp_alloc(sp, &p.P, G * NC, false));
    TRY(sp_alloc(sp, &p.U, G * NC, false));
    TRY(sp_alloc(sp, &p.MV, G * NC, false));
    TRY(sp_alloc(sp, &p.H, G * NC, false));
    TRY(sp_alloc(sp, &p.boards, G * 7168));
    TRY(sp_alloc(sp, &p.meta, G * 8));
    TRY(sp_alloc(sp, &p.legal_mv, G * 224));
    TRY(sp_alloc(sp, &p.legal_idx, G * 224));
    TRY(sp_alloc(sp, &p.n_legal, G));
    TRY(sp_alloc(sp, &p.prior, G * 224));
    TRY(sp_alloc(sp, &p.value, G));
    TRY(sp_alloc(sp, &p.noise, G * 224));
    const size_t T = (size_t)p.trace_cap, S = (size_t)p.num_steps;
    TRY(sp_alloc(sp, &p.thdr, T));
    TRY(sp_alloc(sp, &p.t_move, T * S));
    TRY(sp_alloc(sp, &p.t_q, T * S));
    TRY(sp_alloc(sp, &p.t_nchild, T * S));
    TRY(sp_alloc(sp, &p.t_cmove, T * S * 224, false));
    TRY(sp_alloc(sp, &p.t_cn, T * S * 224, false));
    TRY(sp_alloc(sp, &p.t_cq, T * S * 224, false));
    TRY(sp_alloc(sp, &p.t_cu, T * S * 224, false));
    TRY(sp_alloc(sp, &p.cnt, 1));
    TRY(sp_alloc(sp, &p.slot_cnt, sc::SpParams::slot_cnt_words(G)));
    if (sp->engine && p.evaluator == SC_EVAL_NET) {
        TRY(sp_alloc(sp, &sp->d_hval, G * 64 * 256));
        TRY(sp_alloc(sp, &sp->d_vpart, (size_t)sp->engine->ksplit * G * 128));
        TRY(sp_alloc(sp, &sp->d_fc1_ctr, (G + 63) / 64 * 32));
    }
    // the temperature is fixed for the handle's life (sc_selfplay_set_players / sc_selfplay_set_search do not touch it), and no
    // ply searches more than rollout_num simulations (the cap of --rollout-factor, 300, is rollout_num: create_check)
    if (p.temperature != 0.0f) {
        float* d_w = nullptr;
        const std::vector<float> w = choice_weights(p.temperature, p.rollout);
        TRY(sp_alloc(sp, &d_w, w.size(), false));
        HIPOK(hipMemcpy(d_w, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
        p.choice_w = d_w;
        p.choice_w_max = p.rollout;
    }
    sp->reported.assign((size_t)p.trace_cap, 0);
    return 0;
}

// the network behind the handle, and the form of its step launches
static int create_attach(sc_selfplay* sp) {
    sc_engine* e = sp->engine;
    const sc_selfplay_config& cfg = sp->cfg;
    const bool net = e && cfg.evaluator == SC_EVAL_NET;
    if (e) TRY(engine_reserve(e, cfg.n_slots));
    if (net) {
        sp->p.vf_fused = 1;
        sp->p.vf_ksplit = e->ksplit;
        sp->p.vpart = sp->d_vpart;
        set_value_tail(sp->p, e);
    }
    // (the narrow fp8 tower's workgroup is small enough -- 59 KB of LDS, 249 VGPRs -- for two fused workgroups per CU; the
    // runtime's occupancy answer is used, capped at 2: a third would leave CUs empty at 512 games.  The bf16 one is not.)
    sp->fused = net && !cfg.own_stream && cfg.n_slots <= e->n_cu * e->step_blocks_per_cu;
    // One launch per step: value_head.ffn.0's 64-position tiles are computed by the step kernel's own workgroups (workgroup g:
    // tile (g / 64, K chunk g % 64), step_kernels.hip) -- when the slots fill whole blocks and the split is the kernel's 64.
    sp->fc1_in_step = sp->fused && cfg.n_slots % 64 == 0 && e->ksplit == 64;
    if (sp->fc1_in_step) sp->fc1_in_step = fc1_stream_acquire(sp->device, sp->stream);
    return 0;
}

extern "C" {

int sc_selfplay_create(sc_engine* e, int device_id, const sc_selfplay_config* cfg, sc_selfplay** out) {
    if (!cfg || !out) return fail("null argument");
    *out = nullptr;
    TRY(create_check(e, cfg));
    TRY(use_device(e, device_id));
    // every failure from here on leaves through the guard, that is through sc_selfplay_destroy
    std::unique_ptr<sc_selfplay, void (*)(sc_selfplay*)> guard(new sc_selfplay(), sc_selfplay_destroy);
    sc_selfplay* sp = guard.get();
    sp->engine = e;
    sp->device = e ? e->device : device_id;
    sp->cfg = *cfg;
    if (e && !cfg->own_stream) {
        sp->stream = e->stream;
    } else {
        HIPOK(hipStreamCreateWithFlags(&sp->stream, hipStreamNonBlocking));
        sp->own_stream = true;
    }
    create_params(sp->p, cfg);
    if (create_alloc(sp)) return fail("self-play allocation failed: " + g_err, -2);
    TRY(create_attach(sp));
    scl::init_slots(sp->p, sp->open_lines, sp->stream);
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(sp->stream));
    *out = guard.release();
    return 0;
}

void sc_selfplay_destroy(sc_selfplay* sp) {
    if (!sp) return;
    (void)hipSetDevice(sp->device);
    if (sp->stream) (void)hipStreamSynchronize(sp->stream);
    else (void)hipDeviceSynchronize();
    if (sp->fc1_in_step) fc1_stream_release(sp->device);
    for (void* a : sp->allocs) (void)hipFree(a);
    for (hipEvent_t ev : sp->ev) (void)hipEventDestroy(ev);
    if (sp->ev_begin) (void)hipEventDestroy(sp->ev_begin);
    if (sp->ev_end) (void)hipEventDestroy(sp->ev_end);
    if (sp->enc_ev) {
        (void)hipEventSynchronize(sp->enc_ev);
        (void)hipEventDestroy(sp->enc_ev);
    }
    delete sp->writer;
    sp->d_report.release();
    sp->d_adv.release();
    sp->d_adv_marks.release();
    for (hipEvent_t ev : sp->report_ev)
        if (ev) (void)hipEventDestroy(ev);
    if (sp->own_stream && sp->stream) (void)hipStreamDestroy(sp->stream);
    delete sp;
}

int sc_selfplay_enable_timing(sc_selfplay* sp, int stride) {
    if (!sp) return fail("null handle");
    HIPOK(hipSetDevice(sp->device));
    sp->timing_stride = stride > 0 ? stride : 0;
    sp->step_stride = stride < 0 ? -stride : 0;
    if (stride != 0 && sp->ev.empty()) {
        sp->ev.resize(2 * 4096);
        for (auto& ev : sp->ev) HIPOK(hipEventCreate(&ev));
        HIPOK(hipEventCreate(&sp->ev_begin));
        HIPOK(hipEventCreate(&sp->ev_end));
    }
    return 0;
}

// a sampled launch, or a whole sampled step, between a pair of the handle's 4096 event pairs
static int bracket_begin(sc_selfplay* sp, bool sampled, int* slot) {
    if (!sampled) return 0;
    *slot = sp->ev_next;
    sp->ev_next = (sp->ev_next + 1) % 4096;
    HIPOK(hipEventRecord(sp->ev[2 * *slot], sp->stream));
    return 0;
}
static int bracket_end(sc_selfplay* sp, bool sampled, int slot) {
    if (!sampled) return 0;
    HIPOK(hipEventRecord(sp->ev[2 * slot + 1], sp->stream));
    sp->ev_recorded++;
    return 0;
}

int sc_selfplay_enqueue_sims(sc_selfplay* sp, int n) {
    if (!sp || n < 0) return fail("bad argument");
    if (sp->external) return fail("a handle with an outside opponent is stepped by sc_selfplay_external_search (sc_selfplay_set_external)");
    return sp_enqueue_steps(sp, n);
}

}  // extern "C"

int sp_enqueue_steps(sc_selfplay* sp, int n) {
    if (sp->poisoned) return sp_refuse(sp);
    HIPOK(hipSetDevice(sp->device));
    hipStream_t s = sp->stream;
    const sc::SpParams& p = sp->p;
    const bool any_timing = sp->timing_stride > 0 || sp->step_stride > 0;
    if (any_timing && !sp->have_span) {
        HIPOK(hipEventRecord(sp->ev_begin, s));
        sp->have_span = true;
    }
    for (int i = 0; i < n; i++) {
        sc_engine* e = sp->engine;
        sc::SpParams q = p;
        if (sp->match) {
            // All games are at the same ply: simulation step t belongs to ply t / rollout.  The search kernel first
            // finishes step t-1 (value tail: the weights of THAT step's player), then selects the leaf that this
            // step's player evaluates.
            const int64_t t = sp->sim_steps_enqueued + i;
            const int cur = (int)((t / p.rollout) & 1);
            e = sp->player[cur];
            q.synth_salt = sp->salt[cur];
            match_tail_params(sp, q, t - 1);
            match_search_params(sp, q);
            if (p.match_recycle && t > 0 && t % p.rollout == 0) {
                // a ply boundary: the launch's first half on its own (a no-op where sp_flush has already run it), the games
                // that end and start here, then the launch as usual (nothing is left for its first half to do)
                scl::mcts(q, 1, 0, s);
                match_boundary(sp, t);
            }
        }
        if (p.evaluator != SC_EVAL_NET) {
            scl::mcts(q, 1, 1, s);   // finish the previous simulation (expand/backward/ply transition), select + encode the next leaf
            scl::synth_eval(q, s);
            continue;
        }
        // tower sampling runs the step as separate launches; whole-step sampling (the dominant kernel of production is the step
        // launch itself) does not change the launch form.  sc_selfplay_enable_timing sets one of the two strides at most.
        const bool timed = sp->timing_stride > 0 && (sp->nn_launches % sp->timing_stride) == 0;
        const bool step_timed = sp->step_stride > 0 && (sp->nn_launches % sp->step_stride) == 0;
        const bool one_launch = sp->fused && !timed && sp->fc1_in_step;
        int slot = 0;
        TRY(bracket_begin(sp, step_timed, &slot));
        scnn::TowerArgs t = tower_args(e, p.n_slots, p.boards, p.meta, 8, p.legal_idx, p.n_legal, p.prior, nullptr, sp->d_hval);
        if (sp->fused && !timed) {
            // one launch: the game's search wave (finish the previous simulation, select + encode the next leaf) is wave 0
            // of its tower workgroup (step_kernels.hip); bit-identical to the two launches below
            if (one_launch) {
                t.fc1_arrive = sp->d_fc1_ctr;
                t.fc1_target = 64u * ++sp->fc1_launches + sp->fc1_target_skew;   // every workgroup of a block arrives once per launch (wraps with the counter)
                t.vpart = sp->d_vpart;
                t.fc1_acquire = e->step_blocks_per_cu > 1;
            }
            scl::step(t, q, 1, s);
        } else {
            scl::mcts(q, 1, 1, s);
            // tower only inside the timed bracket: it is the dominant kernel priced by the roofline
            TRY(bracket_begin(sp, timed, &slot));
            scl::tower(t, s);
            TRY(bracket_end(sp, timed, slot));
        }
        // (the tail of the value head is fused into the next search launch)
        if (!one_launch) scl::value_fc1(fc1_args(e, p.n_slots, sp->d_hval, sp->d_vpart), s);
        TRY(bracket_end(sp, step_timed, slot));
        sp->nn_launches++;
    }
    if (n > 0) sp->pending_final = true;  // the last simulation is completed lazily (sp_flush) before any host read
    sp->sim_steps_enqueued += n;
    if (any_timing) HIPOK(hipEventRecord(sp->ev_end, s));
    HIPOK(hipGetLastError());
    return 0;
}

extern "C" {

int sc_selfplay_enqueue_interleaved(sc_selfplay** handles, int n_handles, int n) {
    if (!handles || n_handles <= 0 || n < 0) return fail("bad argument");
    for (int i = 0; i < n; i++)
        for (int h = 0; h < n_handles; h++) TRY(sc_selfplay_enqueue_sims(handles[h], 1));
    return 0;
}

int sc_selfplay_synchronize(sc_selfplay* sp) {
    if (!sp) return fail("null handle");
    return sp_quiesce(sp, true);
}

int sc_selfplay_get_stats(sc_selfplay* sp, sc_selfplay_stats* out) {
    if (!sp || !out) return fail("bad argument");
    TRY(sp_quiesce(sp, false));
    sc::Counters c;
    HIPOK(hipMemcpy(&c, sp->p.cnt, sizeof c, hipMemcpyDeviceToHost));
    std::vector<sc::GameCtl> ctl((size_t)sp->p.n_slots);
    HIPOK(hipMemcpy(ctl.data(), sp->p.ctl, ctl.size() * sizeof(sc::GameCtl), hipMemcpyDeviceToHost));
    int active = 0;
    for (auto& g : ctl) active += g.status == sc::ST_ACTIVE || g.status == sc::ST_PENDING || g.status == sc::ST_MATCH_WAIT;
    std::vector<unsigned long long> sc((size_t)sp->p.n_slots * 2);
    HIPOK(hipMemcpy(sc.data(), sp->p.slot_cnt, sc.size() * 8, hipMemcpyDeviceToHost));
    unsigned long long sims = 0, evals = 0;
    for (int g = 0; g < sp->p.n_slots; g++) {
        sims += sc[(size_t)g * 2];
        evals += sc[(size_t)g * 2 + 1];
    }
    out->sims_done = (int64_t)sims;
    out->nn_evals = (int64_t)evals;
    out->games_finished = c.games_finished;
    out->games_active = active;
    out->error_flags = c.err;
    out->plies_done = (int32_t)c.plies_done;
    return sp_latch(sp);   // (the statistics stay readable on a poisoned handle: that is how the host learns the flags)
}

int sc_selfplay_run(sc_selfplay* sp, int64_t max_sim_steps) {
    if (!sp) return fail("null handle");
    if (sp->p.trace_hold && sp->p.trace_cap < sp->p.total_games)
        return fail("trace_hold with a ring smaller than n_games: drive the handle with sc_selfplay_enqueue_sims + sc_selfplay_poll");
    int64_t done = 0;
    for (;;) {
        int chunk = sp->p.rollout;
        if (max_sim_steps > 0 && done + chunk > max_sim_steps) chunk = (int)(max_sim_steps - done);
        if (chunk <= 0) break;
        TRY(sc_selfplay_enqueue_sims(sp, chunk));
        done += chunk;
        sc_selfplay_stats st;
        TRY(sc_selfplay_get_stats(sp, &st));
        if (sp->poisoned) return sp_refuse(sp);
        if (st.games_active == 0) break;
    }
    return 0;
}

int sc_selfplay_launches_per_step(const sc_selfplay* sp) {
    if (!sp || sp->p.evaluator != SC_EVAL_NET) return 0;
    return sp->fc1_in_step ? 1 : sp->fused ? 2 : 3;
}

int sc_selfplay_timing(sc_selfplay* sp, int reset, float* ms_total, float* ms_nn, int64_t* nn_launches) {
    if (!sp) return fail("null handle");
    TRY(sp_quiesce(sp, false));
    float tot = 0.f, nn = 0.f;
    int64_t cnt = std::min<int64_t>(sp->ev_recorded, 4096);
    if (sp->timing_stride > 0 || sp->step_stride > 0) {
        if (sp->have_span) HIPOK(hipEventElapsedTime(&tot, sp->ev_begin, sp->ev_end));
        for (int64_t k = 0; k < cnt; k++) {
            int slot = (int)(((int64_t)sp->ev_next - 1 - k + 4096 * 2) % 4096);
            float ms = 0.f;
            HIPOK(hipEventElapsedTime(&ms, sp->ev[2 * slot], sp->ev[2 * slot + 1]));
            nn += ms;
        }
    }
    if (ms_total) *ms_total = tot;
    if (ms_nn) *ms_nn = nn;          // sum over the `cnt` sampled tower launches
    if (nn_launches) *nn_launches = cnt;
    if (reset) {
        sp->ev_recorded = 0;
        sp->ev_next = 0;
        sp->have_span = false;
        sp->nn_launches = 0;
    }
    return 0;
}

int sc_selfplay_set_search(sc_selfplay* sp, float cpuct, float epsilon, int with_noise) {
    if (!sp) return fail("null handle");
    if (!(cpuct >= 0.f) || !(epsilon >= 0.f && epsilon <= 1.f)) return fail("bad search parameters");
    // kernel parameters travel by value with every launch: the change applies to the launches enqueued after it
    sp->p.cpuct = cpuct;
    sp->p.epsilon = epsilon;
    sp->p.with_noise = with_noise ? 1 : 0;
    return 0;
}

int sc_selfplay_debug_break_handoff(sc_selfplay* sp, int missing) {
    if (!sp) return fail("null handle");
    if (!sp->fc1_in_step) return 1;
    sp->fc1_target_skew += (uint32_t)missing;
    return 0;
}

int sc_debug_clear_handoff_failure(int device_id) {
    std::lock_guard<std::mutex> lk(g_fc1_mu);
    return std::exchange(g_fc1[device_id].failed, false) ? 0 : 1;
}

}  // extern "C"
