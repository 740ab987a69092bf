// selfplay.hip -- host side of libsc_engine.so: the self-play handle (create, enqueue, statistics, timing, debug entry points).
//
// Step launches that compute value_head.ffn.0 inside the launch (sp->fc1_in_step) make workgroups wait for other workgroups
// of the same launch.  Two such launches running side by side on one device (two streams) could each hold compute units the
// other's late workgroups need: on one device the form is therefore granted to the handles of ONE stream at a time (the first
// to ask; an engine's handles share its stream and run one after the other); any other handle uses the two-launch form.
// (Two PROCESSES sharing a GPU are not covered: the waits are bounded -- error flag 32 -- but one self-play process per GPU
// is the deployment this library is written for.)
#include <math.h>
#include <string.h>

#include <map>
#include <mutex>

#include "host_common.hpp"

static std::mutex g_fc1_mu;
static std::map<int, std::pair<hipStream_t, int>> g_fc1_stream;   // device -> (stream, live handles)
// A device on which an in-launch hand-off has timed out once (the workgroups of a launch were not all resident: someone else
// is using the GPU) is not trusted with that form again by this process: handles created afterwards use the two-launch form,
// whose launches do not wait for each other.
static std::map<int, bool> g_fc1_failed;
static bool fc1_stream_acquire(int device, hipStream_t s) {
    std::lock_guard<std::mutex> lk(g_fc1_mu);
    if (g_fc1_failed.count(device)) return false;
    auto it = g_fc1_stream.find(device);
    if (it == g_fc1_stream.end() || it->second.second == 0) {
        g_fc1_stream[device] = {s, 1};
        return true;
    }
    if (it->second.first != s) return false;
    it->second.second++;
    return true;
}
static void fc1_stream_release(int device) {
    std::lock_guard<std::mutex> lk(g_fc1_mu);
    auto it = g_fc1_stream.find(device);
    if (it != g_fc1_stream.end() && it->second.second > 0) it->second.second--;
}

int sp_refuse(const sc_selfplay*) {
    return fail("an internal hand-off of this handle's step launches timed out (error_flags & 48): its trees and traces are "
                "invalid; destroy the handle -- a new handle on this device uses the two-launch step", SC_ERR_HANDOFF);
}
int sp_latch(sc_selfplay* sp) {
    if (sp->poisoned) return 0;
    int32_t err = 0;
    HIPOK(hipMemcpy(&err, reinterpret_cast<const char*>(sp->p.cnt) + offsetof(sc::Counters, err), 4, hipMemcpyDeviceToHost));
    if (err & (sc::ERR_HELPER_TIMEOUT | sc::ERR_HANDOFF_TIMEOUT)) {
        sp->poisoned = true;
        if (err & sc::ERR_HANDOFF_TIMEOUT) {
            std::lock_guard<std::mutex> lk(g_fc1_mu);
            g_fc1_failed[sp->device] = true;
        }
    }
    return 0;
}

// match play: the value tail of simulation step t uses the weights of the player that evaluated step t
static void match_tail_params(const sc_selfplay* sp, sc::SpParams& q, int64_t t) {
    if (!sp->match || sp->p.evaluator != SC_EVAL_NET || t < 0) return;
    const sc_engine* ep = sp->player[(t / sp->p.rollout) & 1];
    q.vf_w = ep->d_wf;
    q.vf_fc1b = (uint32_t)ep->net.f_fc1b;
    q.vf_fc1m = (uint32_t)ep->net.f_fc1m;
    q.vf_fc2w = (uint32_t)ep->net.f_fc2w;
    q.vf_fc2b = (uint32_t)ep->net.f_fc2b;
}
// Match play with slot recycling.  The search launches never start a game (total_games = 0: a slot whose game ends goes idle);
// games start at the ply boundaries, t % rollout == 0, between the two halves of launch t: after the expansions that end the
// ply, k_match_boundary counts the games that ended and starts those whose White is the player of launch t, (t / rollout) & 1.
static void match_search_params(const sc_selfplay* sp, sc::SpParams& q) {
    if (sp->p.match_recycle) q.total_games = 0;
}
static void match_boundary(const sc_selfplay* sp, int64_t t) {
    sc::SpParams q = sp->p;
    q.match_side = (uint8_t)((t / q.rollout) & 1);
    scl::match_boundary(q, sp->open_lines, sp->stream);
}
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

int sp_opening(const sc_selfplay* sp, int game, const uint16_t** moves) {
    if (sp->open_lines.n <= 0) return 0;
    const size_t i = (size_t)((sp->p.match_colours ? game >> 1 : game) % sp->open_lines.n);
    if (moves) *moves = sp->open_moves.data() + sp->open_move_off[i];
    return (int)(sp->open_move_off[i + 1] - sp->open_move_off[i]);
}
const char* sp_opening_fen(const sc_selfplay* sp, int game) {
    if (sp->open_lines.n <= 0 || sp->open_fens.empty()) return nullptr;
    const size_t i = (size_t)((sp->p.match_colours ? game >> 1 : game) % sp->open_lines.n);
    return sp->open_fens[i].empty() ? nullptr : sp->open_fens[i].c_str();
}

// The weights of the end-of-ply move choice (mcts::step, src/mcts.rs:313-315): w[n] = powf((float)n, 1.0f / temperature) for
// n = 0..n_max, computed HERE, by the host libm -- the function the reference's f32::powf is.  The kernels read the table
// instead of calling the device's powf, whose results differ from the host's in the last bit, because the sampled
// index has to be the reference's bit for bit.
static std::vector<float> choice_weights(float temperature, int n_max) {
    const float power = 1.0f / temperature;
    std::vector<float> w((size_t)n_max + 1);
    for (int n = 0; n <= n_max; n++) w[(size_t)n] = powf((float)n, power);
    return w;
}

template <class T>
static int sp_alloc(sc_selfplay* sp, T** ptr, size_t n, bool zero = true) {
    HIPOK(dalloc(ptr, n));
    sp->allocs.push_back(*ptr);
    if (zero) HIPOK(hipMemset(*ptr, 0, std::max<size_t>(n, 1) * sizeof(T)));
    return 0;
}

extern "C" {

int sc_selfplay_create(sc_engine* e, int device_id, const sc_selfplay_config* cfg, sc_selfplay** out) {
    if (!cfg || !out) return fail("null argument");
    *out = nullptr;
    if (cfg->evaluator == SC_EVAL_NET && !e) return fail("SC_EVAL_NET needs an engine");
    if (cfg->n_slots <= 0 || cfg->n_games <= 0 || cfg->rollout_num < 1 || cfg->num_steps < 1 || cfg->num_steps > 4000)
        return fail("bad self-play configuration");
    if (cfg->rollout_num > 60000) return fail("rollout_num too large");
    if (cfg->evaluator < SC_EVAL_NET || cfg->evaluator > SC_EVAL_SYNTH_UNIFORM) return fail("unknown evaluator");
    if (cfg->rollout_factor < 0.f || (cfg->rollout_factor > 0.f && cfg->rollout_num != 300))
        return fail("rollout_factor needs rollout_num = 300 (the cap of min(300, n_legal * factor), src/main.rs:176)");
    TRY(use_device(e, device_id));
    const int dev = e ? e->device : device_id;
    sc_selfplay* sp = new sc_selfplay();
    sp->engine = e;
    sp->device = dev;
    sp->cfg = *cfg;
    // every failure from here on goes through sc_selfplay_destroy
    auto bail = [&](hipError_t err, const char* what) {
        std::string m = std::string(what) + ": " + hipGetErrorString(err);
        sc_selfplay_destroy(sp);
        return fail(m, -2);
    };
    if (e && !cfg->own_stream) {
        sp->stream = e->stream;
    } else {
        hipError_t he = hipStreamCreateWithFlags(&sp->stream, hipStreamNonBlocking);
        if (he != hipSuccess) {
            sp->stream = nullptr;
            return bail(he, "hipStreamCreate");
        }
        sp->own_stream = true;
    }
    sc::SpParams& p = sp->p;
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
    const size_t G = (size_t)cfg->n_slots, NC = (size_t)p.node_cap;
    int rc = 0;
    rc |= sp_alloc(sp, &p.ctl, G);
    rc |= sp_alloc(sp, &p.hist, G * p.hist_cap, false);
    rc |= sp_alloc(sp, &p.tpos, G * p.tpos_cap, false);
    rc |= sp_alloc(sp, &p.path, G * p.max_depth);
    rc |= sp_alloc(sp, &p.N, G * NC, false);
    rc |= sp_alloc(sp, &p.W, G * NC, false);
    rc |= sp_alloc(sp, &p.P, G * NC, false);
    rc |= sp_alloc(sp, &p.U, G * NC, false);
    rc |= sp_alloc(sp, &p.MV, G * NC, false);
    rc |= sp_alloc(sp, &p.H, G * NC, false);
    rc |= sp_alloc(sp, &p.boards, G * 7168);
    rc |= sp_alloc(sp, &p.meta, G * 8);
    rc |= sp_alloc(sp, &p.legal_mv, G * 224);
    rc |= sp_alloc(sp, &p.legal_idx, G * 224);
    rc |= sp_alloc(sp, &p.n_legal, G);
    rc |= sp_alloc(sp, &p.prior, G * 224);
    rc |= sp_alloc(sp, &p.value, G);
    rc |= sp_alloc(sp, &p.noise, G * 224);
    const size_t T = (size_t)p.trace_cap, S = (size_t)p.num_steps;
    rc |= sp_alloc(sp, &p.thdr, T);
    rc |= sp_alloc(sp, &p.t_move, T * S);
    rc |= sp_alloc(sp, &p.t_q, T * S);
    rc |= sp_alloc(sp, &p.t_nchild, T * S);
    rc |= sp_alloc(sp, &p.t_cmove, T * S * 224, false);
    rc |= sp_alloc(sp, &p.t_cn, T * S * 224, false);
    rc |= sp_alloc(sp, &p.t_cq, T * S * 224, false);
    rc |= sp_alloc(sp, &p.t_cu, T * S * 224, false);
    rc |= sp_alloc(sp, &p.cnt, 1);
    rc |= sp_alloc(sp, &p.slot_cnt, sc::SpParams::slot_cnt_words(G));
    // the temperature is fixed for the handle's life (sc_selfplay_set_players / sc_selfplay_set_search do not touch it), and no
    // ply searches more than rollout_num simulations (the cap of --rollout-factor, 300, is rollout_num: checked above)
    float* d_choice_w = nullptr;
    if (cfg->temperature != 0.0f) rc |= sp_alloc(sp, &d_choice_w, (size_t)cfg->rollout_num + 1, false);
    if (rc) {
        std::string keep = g_err;
        sc_selfplay_destroy(sp);
        return fail("self-play allocation failed: " + keep, -2);
    }
    if (d_choice_w) {
        const std::vector<float> w = choice_weights(cfg->temperature, cfg->rollout_num);
        hipError_t he = hipMemcpy(d_choice_w, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice);
        if (he != hipSuccess) return bail(he, "hipMemcpy(choice weights)");
        p.choice_w = d_choice_w;
        p.choice_w_max = cfg->rollout_num;
    }
    if (e) {
        rc = engine_reserve(e, cfg->n_slots);
        if (rc) {
            sc_selfplay_destroy(sp);
            return rc;
        }
    }
    if (e && cfg->evaluator == SC_EVAL_NET) {
        rc |= sp_alloc(sp, &sp->d_hval, G * 64 * 256);
        rc |= sp_alloc(sp, &sp->d_vpart, (size_t)e->ksplit * G * 128);
        rc |= sp_alloc(sp, &sp->d_fc1_ctr, (G + 63) / 64 * 32);
        if (rc) {
            sc_selfplay_destroy(sp);
            return fail("self-play allocation failed", -2);
        }
        p.vf_fused = 1;
        p.vf_ksplit = e->ksplit;
        p.vpart = sp->d_vpart;
        p.vf_w = e->d_wf;
        p.vf_fc1b = (uint32_t)e->net.f_fc1b;
        p.vf_fc1m = (uint32_t)e->net.f_fc1m;
        p.vf_fc2w = (uint32_t)e->net.f_fc2w;
        p.vf_fc2b = (uint32_t)e->net.f_fc2b;
    }
    sp->reported.assign((size_t)p.trace_cap, 0);
    // (the narrow fp8 tower's workgroup is small enough -- 59 KB of LDS, 249 VGPRs -- for two fused workgroups per CU; the
    // runtime's occupancy answer is used, capped at 2: a third would leave CUs empty at 512 games.  The bf16 one is not.)
    sp->fused = e && cfg->evaluator == SC_EVAL_NET && !cfg->own_stream && cfg->n_slots <= e->n_cu * e->step_blocks_per_cu;
#ifdef SC_EXP
    if (getenv("SC_FUSED")) sp->fused = getenv("SC_FUSED")[0] != '0';   // experiment builds: A/B
#endif
    // One launch per step: value_head.ffn.0's 64-position tiles are computed by the step kernel's own workgroups (workgroup g:
    // tile (g / 64, K chunk g % 64), step_kernels.hip) -- when the slots fill whole blocks and the split is the kernel's 64.
    sp->fc1_in_step = sp->fused && cfg->n_slots % 64 == 0 && e->ksplit == 64;
#ifdef SC_FC1_IN_STEP_OFF   // A/B builds
    sp->fc1_in_step = false;
#endif
    if (sp->fc1_in_step) sp->fc1_in_step = fc1_stream_acquire(sp->device, sp->stream);
    // the zero-fills above ran on the NULL stream, which does not order against the (non-blocking) launch
    // stream: make them complete before the first kernel touches the buffers
    hipError_t he = hipDeviceSynchronize();
    if (he != hipSuccess) return bail(he, "hipDeviceSynchronize");
    scl::init_slots(p, sp->open_lines, sp->stream);
    if ((he = hipGetLastError()) != hipSuccess) return bail(he, "k_init_slots");
    if ((he = hipStreamSynchronize(sp->stream)) != hipSuccess) return bail(he, "k_init_slots");
    *out = sp;
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

int sc_selfplay_set_players(sc_selfplay* sp, sc_engine* white, sc_engine* black, uint64_t salt_white, uint64_t salt_black) {
    if (!sp) return fail("null handle");
    if (sp->sim_steps_enqueued != 0) return fail("set_players must precede the first enqueue");
    if (sp->cfg.n_games != sp->cfg.n_slots) return fail("match play needs n_games == n_slots (lockstep plies, no slot recycling)");
    if (sp->cfg.rollout_factor > 0.f) return fail("match play needs a fixed rollout (lockstep plies)");
    if (sp->cfg.evaluator == SC_EVAL_NET) {
        if (!white || !black) return fail("match play with SC_EVAL_NET needs two engines");
        if (white->device != sp->device || black->device != sp->device) return fail("both engines must live on the handle's device");
        if (white->ksplit != sp->engine->ksplit || black->ksplit != sp->engine->ksplit) return fail("engines differ in split-K");
        TRY(engine_reserve(white, sp->cfg.n_slots));
        TRY(engine_reserve(black, sp->cfg.n_slots));
    }
    sp->match = true;
    sp->player[0] = white;
    sp->player[1] = black;
    sp->salt[0] = salt_white;
    sp->salt[1] = salt_black;
    return 0;
}

// sc_selfplay_set_players' preconditions on the rollout and the engines (not its n_games == n_slots)
static int match_players_check(sc_selfplay* sp, sc_engine* a, sc_engine* b) {
    if (sp->cfg.rollout_factor > 0.f) return fail("match play needs a fixed rollout (lockstep plies)");
    if (sp->cfg.evaluator == SC_EVAL_NET) {
        if (!a || !b) return fail("match play with SC_EVAL_NET needs two engines");
        if (a->device != sp->device || b->device != sp->device) return fail("both engines must live on the handle's device");
        if (a->ksplit != sp->engine->ksplit || b->ksplit != sp->engine->ksplit) return fail("engines differ in split-K");
        TRY(engine_reserve(a, sp->cfg.n_slots));
        TRY(engine_reserve(b, sp->cfg.n_slots));
    }
    return 0;
}

int sc_selfplay_set_match(sc_selfplay* sp, sc_engine* a, sc_engine* b, uint64_t salt_a, uint64_t salt_b, int colours) {
    if (!sp) {
        TRY(use_device(nullptr, 0));
        return fail("null handle");
    }
    if (sp->poisoned) return sp_refuse(sp);
    if (sp->sim_steps_enqueued != 0 || sp->match) return fail("set_match must precede the first enqueue (and any other choice of players)");
    if (colours != 0 && colours != 1) return fail("set_match: colours must be 0 (a is White in every game) or 1 (a and b alternate as White)");
    TRY(match_players_check(sp, a, b));
    HIPOK(hipSetDevice(sp->device));
    sc::SpParams& p = sp->p;
    TRY(sp_alloc(sp, &sp->d_match_sum, 8));
    // With alternating colours a game waits for its ring row's previous game, cap ordinals back: of the SAME side only if cap is
    // even, and then drawn before it.  An odd ring could leave every slot waiting for games of the other side that no slot is
    // left to draw.
    if (colours && p.trace_cap < p.total_games && (p.trace_cap & 1)) p.trace_cap -= 1;   // (>= 2 * n_slots still)
    // The slots were set up for plain self-play (sc_selfplay_create: slot g plays game g).  Nothing has run since: take that
    // back and set them up again by the match's start rule.
    HIPOK(hipDeviceSynchronize());   // (the zero-fills above ran on the NULL stream)
    HIPOK(hipMemsetAsync(p.cnt, 0, sizeof(sc::Counters), sp->stream));
    HIPOK(hipMemsetAsync(p.ctl, 0, (size_t)p.n_slots * sizeof(sc::GameCtl), sp->stream));
    HIPOK(hipMemsetAsync(p.thdr, 0, (size_t)p.trace_cap * sizeof(sc::TraceHdr), sp->stream));
    p.match_recycle = 1;
    p.match_colours = (uint8_t)colours;
    scl::init_slots(p, sp->open_lines, sp->stream);   // (match_side = 0: the boundary of ply 0; no lines yet)
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(sp->stream));
    sp->match = true;
    sp->player[0] = a;
    sp->player[1] = b;
    sp->salt[0] = salt_a;
    sp->salt[1] = salt_b;
    return 0;
}

// The lines are replayed and checked ONCE, here (k_open_lines), into records that stay on the device; a game start copies its line's
// records into the slot (k_match_boundary).  Nothing has run on the handle yet: as sc_selfplay_set_match does, the slots' initial
// draw is taken back and made again, now with the lines.
int sc_selfplay_set_openings(sc_selfplay* sp, int n_lines, const uint16_t* moves, const uint32_t* move_off, int32_t* status) {
    return sc_selfplay_set_openings_from(sp, n_lines, nullptr, nullptr, moves, move_off, status);
}

// ... with a base per line.  The start rule lives in k_match_boundary, which reads it off the line's record count: the first
// searched ply of a line of `len + 1` records belongs to player white(k) ^ (len & 1), and a line of one record is not copied at all
// (the slot already holds the start position).  That kernel stays as it is.  A base makes the host choose the record count
// instead: `pad` empty records in front of the base, so that len = pad + L is odd exactly when Black is to move in the line's
// last position, and at least 1 -- one record for a base with Black to move, two for a base with White to move and no moves.
// k_open_lines writes them (no men, no flags: zero planes) and marks the base F_IRREV, where every repetition scan stops.
int sc_selfplay_set_openings_from(sc_selfplay* sp, int n_lines, const sc_positions* bases, const int32_t* base_idx, const uint16_t* moves,
                                  const uint32_t* move_off, int32_t* status) {
    if (!sp) return fail("null handle");
    if (sp->poisoned) return sp_refuse(sp);
    if (!sp->p.match_recycle) return fail("set_openings needs a handle set up by sc_selfplay_set_match");
    if (sp->sim_steps_enqueued != 0) return fail("set_openings must precede the first enqueue");
    if (n_lines < 1 || !move_off) return fail("set_openings: bad argument");
    sc::SpParams& p = sp->p;
    if (!bases || !base_idx) {
        bases = nullptr;
        base_idx = nullptr;
    }
    if (bases) {
        if (bases->device != sp->device) return fail("set_openings: the positions live on another device than the handle");
        if (status) std::fill(status, status + n_lines, 0);
        int bad = -1;
        for (int i = 0; i < n_lines; i++) {
            const int b = base_idx[i];
            if (b >= bases->n) return fail("set_openings: base index " + std::to_string(b) + " of " + std::to_string(bases->n) + " positions");
            if (b >= 0 && bases->status[(size_t)b] != 0) {
                if (status) status[i] = bases->status[(size_t)b];
                if (bad < 0) bad = i;
            }
        }
        if (bad >= 0)
            return fail("set_openings: the base of line " + std::to_string(bad) + " has status " + std::to_string(bases->status[(size_t)base_idx[bad]]) +
                        (bases->status[(size_t)base_idx[bad]] < 0 ? " (it cannot be played)" : " (the game is over there)"));
    }
    std::vector<uint32_t> rec_off((size_t)n_lines + 1, 0);
    for (int i = 0; i < n_lines; i++) {
        if (move_off[i + 1] < move_off[i]) return fail("set_openings: move_off must not decrease");
        const uint32_t len = move_off[i + 1] - move_off[i];
        uint32_t pad = 0;
        if (bases && base_idx[i] >= 0) {
            const bool black_last = (bases->rec[(size_t)base_idx[i]].turn == sc::BLACK) != ((len & 1) != 0);
            pad = ((len & 1) != 0) == black_last ? 0 : 1;
            if (pad + len == 0) pad = 2;
        }
        if (len > 600 || (int64_t)pad + len + 1 > (int64_t)p.hist_cap)
            return fail("set_openings: line " + std::to_string(i) + " has " + std::to_string(len) + " plies (at most 600)");
        rec_off[(size_t)i + 1] = rec_off[(size_t)i] + pad + len + 1;
        if ((size_t)rec_off[(size_t)i + 1] * sizeof(sc::Position) > ((size_t)1 << 30))
            return fail("set_openings: the lines' position records exceed 1 GiB");
    }
    const size_t n_moves = move_off[n_lines], first = move_off[0], n_rec = rec_off[(size_t)n_lines];
    if (n_moves > first && !moves) return fail("set_openings: bad argument");
    if (status) std::fill(status, status + n_lines, 0);
    HIPOK(hipSetDevice(sp->device));
    ScopedDev<uint16_t> d_moves;
    ScopedDev<uint32_t> d_moff, d_roff;
    ScopedDev<int32_t> d_status, d_bidx;
    ScopedDev<sc::Position> d_tab;
    if (bases) {
        HIPOK(d_bidx.alloc((size_t)n_lines));
        HIPOK(hipMemcpy(d_bidx.p, base_idx, (size_t)n_lines * 4, hipMemcpyHostToDevice));
    }
    HIPOK(d_moves.alloc(n_moves));
    HIPOK(d_moff.alloc((size_t)n_lines + 1));
    HIPOK(d_roff.alloc((size_t)n_lines + 1));
    HIPOK(d_status.alloc((size_t)n_lines));
    HIPOK(d_tab.alloc(n_rec));
    if (n_moves) HIPOK(hipMemcpy(d_moves.p, moves, n_moves * 2, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_moff.p, move_off, ((size_t)n_lines + 1) * 4, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_roff.p, rec_off.data(), ((size_t)n_lines + 1) * 4, hipMemcpyHostToDevice));
    scl::open_lines(n_lines, d_moves.p, d_moff.p, d_tab.p, d_roff.p, d_status.p, {bases ? bases->d_rec : nullptr, d_bidx.p}, sp->stream);
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(sp->stream));
    std::vector<int32_t> st((size_t)n_lines);
    HIPOK(hipMemcpy(st.data(), d_status.p, (size_t)n_lines * 4, hipMemcpyDeviceToHost));
    if (status) std::copy(st.begin(), st.end(), status);
    for (int i = 0; i < n_lines; i++)
        if (st[(size_t)i] != 0)
            return fail("set_openings: line " + std::to_string(i) + " has status " + std::to_string(st[(size_t)i]) +
                        (st[(size_t)i] < 0 ? " (move " + std::to_string(-st[(size_t)i] - 1) + " is not legal)" : " (the game is over at its end)"));
    // accepted: the slots' initial draw again, on the fresh state (sc_selfplay_set_match)
    HIPOK(hipMemsetAsync(p.cnt, 0, sizeof(sc::Counters), sp->stream));
    HIPOK(hipMemsetAsync(p.ctl, 0, (size_t)p.n_slots * sizeof(sc::GameCtl), sp->stream));
    HIPOK(hipMemsetAsync(p.thdr, 0, (size_t)p.trace_cap * sizeof(sc::TraceHdr), sp->stream));
    const sc::MatchLines lines{d_tab.p, d_roff.p, n_lines};
    scl::init_slots(p, lines, sp->stream);
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(sp->stream));
    // (a second call replaces the table of the first)
    for (const void* old : {(const void*)sp->open_lines.tab, (const void*)sp->open_lines.off}) {
        auto it = std::find(sp->allocs.begin(), sp->allocs.end(), old);
        if (old && it != sp->allocs.end()) {
            (void)hipFree(*it);
            sp->allocs.erase(it);
        }
    }
    sp->open_lines = lines;
    sp->allocs.push_back(d_tab.p);
    sp->allocs.push_back(d_roff.p);
    d_tab.p = nullptr;
    d_roff.p = nullptr;
    sp->open_moves.clear();
    if (n_moves > first) sp->open_moves.assign(moves + first, moves + n_moves);
    sp->open_move_off.resize((size_t)n_lines + 1);
    for (int i = 0; i <= n_lines; i++) sp->open_move_off[(size_t)i] = move_off[i] - (uint32_t)first;
    sp->open_fens.clear();
    if (bases) {
        sp->open_fens.resize((size_t)n_lines);
        for (int i = 0; i < n_lines; i++)
            if (base_idx[i] >= 0) sp->open_fens[(size_t)i] = position_fen(bases->rec[(size_t)base_idx[i]], bases->ep_legal[(size_t)base_idx[i]] != 0);
    }
    return 0;
}

int sc_selfplay_get_opening_fen(sc_selfplay* sp, int game, char* buf, int cap) {
    if (!sp) return fail("null handle");
    if (game < 0 || game >= sp->cfg.n_games || cap < 0 || (cap > 0 && !buf)) return fail("bad argument");
    const char* fen = sp_opening_fen(sp, game);
    const std::string s = fen ? fen : "";
    if (cap > 0) {
        const size_t k = std::min(s.size(), (size_t)cap - 1);
        memcpy(buf, s.data(), k);
        buf[k] = 0;
    }
    return (int)s.size();
}

int sc_selfplay_get_opening(sc_selfplay* sp, int game, uint16_t* moves, int cap) {
    if (!sp) return fail("null handle");
    if (game < 0 || game >= sp->cfg.n_games || cap < 0 || (cap > 0 && !moves)) return fail("bad argument");
    const uint16_t* mv = nullptr;
    const int len = sp_opening(sp, game, &mv);
    for (int i = 0; i < len && i < cap; i++) moves[i] = mv[i];
    return len;
}

int sc_selfplay_match_tally(sc_selfplay* sp, int64_t out[8]) {
    if (!sp) {
        TRY(use_device(nullptr, 0));
        return fail("null handle");
    }
    if (!out) return fail("null argument");
    if (!sp->p.match_recycle) return fail("match_tally needs a handle set up by sc_selfplay_set_match");
    TRY(sp_quiesce(sp, true));
    scl::match_tally(sp->p.match_tally(), sp->p.n_slots, sp->d_match_sum, sp->stream);
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(sp->stream));
    static_assert(sizeof(long long) == sizeof(int64_t), "the reduction kernel writes int64");
    HIPOK(hipMemcpy(out, sp->d_match_sum, 8 * sizeof(int64_t), hipMemcpyDeviceToHost));
    return 0;
}

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
    return g_fc1_failed.erase(device_id) ? 0 : 1;
}

int sc_debug_find_max(int device_id, const float* values, int n, int32_t* out2) {
    if (!values || !out2 || n < 1 || n > 256) return fail("bad argument");
    TRY(use_device(nullptr, device_id));
    ScopedDev<float> d_u;
    ScopedDev<int> d_o;
    HIPOK(d_u.alloc(256));
    HIPOK(d_o.alloc(2));
    HIPOK(hipMemcpy(d_u.p, values, (size_t)n * 4, hipMemcpyHostToDevice));
    scl::debug_find_max(d_u.p, n, d_o.p, nullptr);
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpy(out2, d_o.p, 8, hipMemcpyDeviceToHost));
    return 0;
}

int sc_debug_choose_child(int device_id, int n_cases, const int32_t* n_act, const int32_t* nc, const float* temperature, const float* u,
                          int tie_random, int32_t* choice_out, float* total_out) {
    if (!n_act || !nc || !temperature || !u || !choice_out || !total_out || n_cases < 1 || n_cases > (1 << 20)) return fail("bad argument");
    int w_max = 0;
    for (int c = 0; c < n_cases; c++) {
        if (nc[c] < 1 || nc[c] > sc::MAXC) return fail("sc_debug_choose_child: nc out of [1, 224]");
        if (!(temperature[c] >= 0.0f) || !(u[c] >= 0.0f && u[c] < 1.0f)) return fail("sc_debug_choose_child: temperature < 0 or u outside [0, 1)");
        for (int i = 0; i < nc[c]; i++) {
            const int32_t n = n_act[(size_t)c * sc::MAXC + i];
            if (n < 0 || n > 60000) return fail("sc_debug_choose_child: visit count out of [0, 60000]");
            w_max = std::max(w_max, (int)n);
        }
    }
    // one weight table per distinct temperature, made by the function that makes a self-play handle's
    std::vector<float> w(1, 0.0f);
    std::vector<int32_t> w_off((size_t)n_cases, 0);
    std::map<uint32_t, int32_t> table_of;
    for (int c = 0; c < n_cases; c++) {
        if (temperature[c] == 0.0f) continue;
        uint32_t bits;
        memcpy(&bits, &temperature[c], 4);
        auto it = table_of.find(bits);
        if (it == table_of.end()) {
            if (table_of.size() >= 64) return fail("sc_debug_choose_child: more than 64 distinct temperatures");
            it = table_of.emplace(bits, (int32_t)w.size()).first;
            const std::vector<float> t = choice_weights(temperature[c], w_max);
            w.insert(w.end(), t.begin(), t.end());
        }
        w_off[(size_t)c] = it->second;
    }
    TRY(use_device(nullptr, device_id));
    const size_t n = (size_t)n_cases;
    ScopedDev<int32_t> d_n, d_nc, d_ch, d_off;
    ScopedDev<float> d_t, d_u, d_tot, d_w;
    HIPOK(d_n.alloc(n * sc::MAXC));
    HIPOK(d_nc.alloc(n));
    HIPOK(d_ch.alloc(n));
    HIPOK(d_off.alloc(n));
    HIPOK(d_t.alloc(n));
    HIPOK(d_u.alloc(n));
    HIPOK(d_tot.alloc(n));
    HIPOK(d_w.alloc(w.size()));
    HIPOK(hipMemcpy(d_n.p, n_act, n * sc::MAXC * 4, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_nc.p, nc, n * 4, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_t.p, temperature, n * 4, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_u.p, u, n * 4, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_off.p, w_off.data(), n * 4, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_w.p, w.data(), w.size() * 4, hipMemcpyHostToDevice));
    scl::debug_choose_child(n_cases, d_n.p, d_nc.p, d_t.p, d_u.p, tie_random ? 1 : 0, d_w.p, d_off.p, w_max, d_ch.p, d_tot.p, nullptr);
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpy(choice_out, d_ch.p, n * 4, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(total_out, d_tot.p, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

/* developer aid: cycle stamps of the last k_mcts launch, out[n_slots][8] */
int sc_selfplay_debug_cycles(sc_selfplay* sp, int enable, unsigned long long* out) {
    if (!sp) return fail("null handle");
    HIPOK(hipSetDevice(sp->device));
    HIPOK(hipStreamSynchronize(sp->stream));
    if (enable && !sp->p.dbg_cycles) {
        HIPOK(dalloc(&sp->p.dbg_cycles, (size_t)sp->p.n_slots * 32));
        sp->allocs.push_back(sp->p.dbg_cycles);
        HIPOK(hipMemset(sp->p.dbg_cycles, 0, (size_t)sp->p.n_slots * 256));
        HIPOK(hipDeviceSynchronize());
    }
    if (out && sp->p.dbg_cycles)
        HIPOK(hipMemcpy(out, sp->p.dbg_cycles, (size_t)sp->p.n_slots * 256, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
