// external_play.hip -- host side of libsc_engine.so: match play against an outside opponent (the reference's `play --black-type
// stockfish`, src/play.rs:38-59, 89-142).  The handle searches the engine's plies; the opponent's moves arrive from the host and
// are played on the device in many slots at once (external_kernels.hip).  A round: sc_selfplay_external_wait lists the slots that
// wait, the host asks the opponent, sc_selfplay_push_moves plays the answers; when no slot waits, sc_selfplay_external_search
// searches one ply of every live game.  No search kernel knows of this: they get total_games = 0 and the boundary kernels run here.
#include "host_common.hpp"

// the device arrays of the wait kernel and of a push, [n_slots] each: made once, by the first call that needs them
static int ext_buffers(sc_selfplay* sp) {
    if (sp->d_ext_list) return 0;
    const size_t G = (size_t)sp->p.n_slots;
    TRY(sp_alloc(sp, &sp->d_ext_list, G));
    TRY(sp_alloc(sp, &sp->d_ext_count, 1));
    TRY(sp_alloc(sp, &sp->d_ext_epl, G));
    TRY(sp_alloc(sp, &sp->d_ext_recs, G));
    TRY(sp_alloc(sp, &sp->d_ext_info, G));
    TRY(sp_alloc(sp, &sp->d_push_slots, G));
    TRY(sp_alloc(sp, &sp->d_push_moves, G));
    TRY(sp_alloc(sp, &sp->d_push_status, G));
    return 0;
}

// completes the handle's work, runs k_external_wait and brings the count over: *n slots wait (their entries stay on the device)
static int ext_wait_count(sc_selfplay* sp, int* n) {
    TRY(sp_quiesce(sp, true));
    TRY(ext_buffers(sp));
    scl::external_wait(sp->p, sp->external, sp->d_ext_list, sp->d_ext_count, sp->d_ext_recs, sp->d_ext_epl, sp->d_ext_info, sp->stream);
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(sp->stream));
    int32_t count = 0;
    HIPOK(hipMemcpy(&count, sp->d_ext_count, 4, hipMemcpyDeviceToHost));
    if (count < 0 || count > sp->p.n_slots) return fail("external_wait: bad count from the device");
    *n = count;
    sp->ext_waiting = count;
    return 0;
}

extern "C" {

int sc_selfplay_set_external(sc_selfplay* sp, sc_engine* engine, uint64_t synth_salt, int colours) {
    if (!sp) {
        TRY(use_device(nullptr, 0));
        return fail("null handle");
    }
    if (sp->poisoned) return sp_refuse(sp);
    if (sp->sim_steps_enqueued != 0 || sp->match || sp->external)
        return fail("set_external must precede the first enqueue (and any other choice of players)");
    if (colours < 0 || colours > 2) return fail("set_external: colours must be 0 (the engine is White in every game), 1 (White in the even games) or 2 (Black in every game)");
    if (sp->cfg.rollout_factor > 0.f) return fail("set_external needs a fixed rollout (every live game ends its ply in the same launch)");
    if (sp->cfg.outcome_gate != -1) return fail("set_external needs outcome_gate = -1: the opponent is never handed a finished position (src/play.rs:335)");
    sc_engine* e = engine ? engine : sp->engine;
    if (sp->cfg.evaluator == SC_EVAL_NET) {
        if (!e) return fail("set_external with SC_EVAL_NET needs an engine");
        if (e->device != sp->device) return fail("the engine must live on the handle's device");
        if (e->ksplit != sp->engine->ksplit) return fail("engines differ in split-K");
        TRY(engine_reserve(e, sp->cfg.n_slots));
    }
    HIPOK(hipSetDevice(sp->device));
    sc::SpParams& p = sp->p;
    TRY(sp_alloc(sp, &sp->d_match_sum, 8));
    TRY(ext_buffers(sp));
    // Nothing has run on the handle yet: the slots' initial draw (sc_selfplay_create: slot g plays game g) is taken back as
    // sc_selfplay_set_match takes it back -- k_init_slots under the match rule with no game to draw leaves every slot idle -- and
    // the first games start under the boundary rule
    HIPOK(hipMemsetAsync(p.cnt, 0, sizeof(sc::Counters), sp->stream));
    HIPOK(hipMemsetAsync(p.ctl, 0, (size_t)p.n_slots * sizeof(sc::GameCtl), sp->stream));
    HIPOK(hipMemsetAsync(p.thdr, 0, (size_t)p.trace_cap * sizeof(sc::TraceHdr), sp->stream));
    sc::SpParams q = p;
    q.match_recycle = 1;
    q.total_games = 0;
    scl::init_slots(q, sp->open_lines, sp->stream);
    HIPOK(hipMemsetAsync(p.cnt, 0, sizeof(sc::Counters), sp->stream));   // (every slot has drawn an ordinal there, in vain)
    scl::external_boundary(p, 1 + colours, sp->stream);
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(sp->stream));
    // one player on every ply that is searched: the stepping loop's match form with both seats the engine's
    sp->match = true;
    sp->player[0] = sp->player[1] = e;
    sp->salt[0] = sp->salt[1] = synth_salt;
    sp->external = 1 + colours;
    sp->ext_waiting = -1;
    return 0;
}

int sc_selfplay_external_search(sc_selfplay* sp) {
    if (!sp) return fail("null handle");
    if (!sp->external) return fail("external_search needs a handle set up by sc_selfplay_set_external");
    if (sp->poisoned) return sp_refuse(sp);
    if (sp->ext_waiting < 0) {   // (a fresh handle, or moves pushed since the last look)
        int n = 0;
        TRY(ext_wait_count(sp, &n));
    }
    if (sp->ext_waiting > 0)
        return fail("external_search: " + std::to_string(sp->ext_waiting) + " slots wait for the opponent's move (sc_selfplay_external_wait, sc_selfplay_push_moves)");
    TRY(sp_enqueue_steps(sp, sp->p.rollout));
    sp_flush(sp);   // the expansions that end the ply
    scl::external_boundary(sp->p, sp->external, sp->stream);
    HIPOK(hipGetLastError());
    sp->ext_waiting = -1;
    return 0;
}

int sc_selfplay_external_wait(sc_selfplay* sp, int cap, int32_t* slots, int32_t* games, int32_t* plies, char* fens, uint64_t fens_cap,
                              uint32_t* fen_off, uint16_t* moves, uint32_t moves_cap, uint32_t* move_off) {
    if (!sp || cap < 0) return fail("bad argument");
    if (!sp->external) return fail("external_wait needs a handle set up by sc_selfplay_set_external");
    if (sp->poisoned) return sp_refuse(sp);
    int n = 0;
    TRY(ext_wait_count(sp, &n));
    if (n == 0) {
        if (fen_off) fen_off[0] = 0;
        if (move_off) move_off[0] = 0;
        return 0;
    }
    if ((slots || games || plies || fen_off || move_off || fens || moves) && n > cap)
        return fail("external_wait: " + std::to_string(n) + " slots wait, the arrays hold " + std::to_string(cap));
    const sc::SpParams& p = sp->p;
    std::vector<int32_t> list((size_t)n), epl((size_t)n);
    std::vector<sc::Position> recs((size_t)n);
    std::vector<int4> info((size_t)n);
    HIPOK(hipMemcpy(list.data(), sp->d_ext_list, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(recs.data(), sp->d_ext_recs, (size_t)n * sizeof(sc::Position), hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(epl.data(), sp->d_ext_epl, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(info.data(), sp->d_ext_info, (size_t)n * sizeof(int4), hipMemcpyDeviceToHost));
    // everything is sized before anything is written
    std::string text;
    std::vector<uint32_t> foff((size_t)n + 1, 0), moff((size_t)n + 1, 0);
    if (fens || fen_off) {
        for (int i = 0; i < n; i++) {
            text += position_fen(recs[(size_t)i], epl[(size_t)i] != 0);
            text += '\0';
            foff[(size_t)i + 1] = (uint32_t)text.size();
        }
        if (fens && text.size() > fens_cap)
            return fail("external_wait: the FENs take " + std::to_string(text.size()) + " bytes, the buffer holds " + std::to_string(fens_cap));
    }
    std::vector<uint16_t> mv;
    if (moves || move_off) {
        for (int i = 0; i < n; i++) {
            const int4& f = info[(size_t)i];
            if (f.z < 0 || f.z >= p.trace_cap || f.w < 0 || f.w > p.num_steps) return fail("external_wait: bad trace row from the device");
            moff[(size_t)i + 1] = moff[(size_t)i] + (uint32_t)f.w;
        }
        if (moves && moff[(size_t)n] > moves_cap)
            return fail("external_wait: the move lists take " + std::to_string(moff[(size_t)n]) + " moves, the buffer holds " + std::to_string(moves_cap));
        if (moves) {
            mv.resize((size_t)moff[(size_t)n] + 1);
            for (int i = 0; i < n; i++)   // the played moves of the live trace row
                if (info[(size_t)i].w > 0)
                    HIPOK(hipMemcpy(mv.data() + moff[(size_t)i], p.t_move + (size_t)info[(size_t)i].z * p.num_steps, (size_t)info[(size_t)i].w * 2,
                                    hipMemcpyDeviceToHost));
        }
    }
    for (int i = 0; i < n; i++) {
        if (slots) slots[i] = list[(size_t)i];
        if (games) games[i] = info[(size_t)i].x;
        if (plies) plies[i] = info[(size_t)i].y;
    }
    if (fens) std::copy(text.begin(), text.end(), fens);
    if (fen_off) std::copy(foff.begin(), foff.end(), fen_off);
    if (moves) std::copy(mv.begin(), mv.begin() + moff[(size_t)n], moves);
    if (move_off) std::copy(moff.begin(), moff.end(), move_off);
    return n;
}

int sc_selfplay_push_moves(sc_selfplay* sp, int n, const int32_t* slots, const uint16_t* moves, int32_t* status) {
    if (!sp || n < 0 || (n > 0 && (!slots || !moves))) return fail("bad argument");
    if (sp->poisoned) return sp_refuse(sp);
    if (n == 0) return 0;
    const sc::SpParams& p = sp->p;
    std::vector<char> seen((size_t)p.n_slots, 0);
    for (int i = 0; i < n; i++) {
        if (slots[i] < 0 || slots[i] >= p.n_slots) return fail("push_moves: slot " + std::to_string(slots[i]) + " of " + std::to_string(p.n_slots));
        if (seen[(size_t)slots[i]]) return fail("push_moves: slot " + std::to_string(slots[i]) + " is listed twice");
        seen[(size_t)slots[i]] = 1;
    }
    TRY(sp_quiesce(sp, true));
    TRY(ext_buffers(sp));
    HIPOK(hipMemcpyAsync(sp->d_push_slots, slots, (size_t)n * 4, hipMemcpyHostToDevice, sp->stream));
    HIPOK(hipMemcpyAsync(sp->d_push_moves, moves, (size_t)n * 2, hipMemcpyHostToDevice, sp->stream));
    // a game that a pushed move ends is finished under the handle's own rule: a recycled or external slot goes idle and its
    // boundary kernel takes over, any other slot draws the next game at once
    sc::SpParams q = p;
    if (p.match_recycle || sp->external) q.total_games = 0;
    scl::push_moves(q, n, sp->d_push_slots, sp->d_push_moves, sp->d_push_status, sp->external, sp->stream);
    if (sp->external) scl::external_boundary(p, sp->external, sp->stream);
    HIPOK(hipGetLastError());
    std::vector<int32_t> st((size_t)n);
    HIPOK(hipMemcpyAsync(st.data(), sp->d_push_status, (size_t)n * 4, hipMemcpyDeviceToHost, sp->stream));
    HIPOK(hipStreamSynchronize(sp->stream));
    sp->ext_waiting = -1;
    int refused = 0;
    for (int i = 0; i < n; i++) refused += st[(size_t)i] < 0;
    if (status) std::copy(st.begin(), st.end(), status);
    return refused;
}

}  // extern "C"
