// match_play.hip -- host side of libsc_engine.so: match set-up of a self-play handle (the lockstep form, the form that recycles
// slots, opening lines with or without a base) and its read-backs.  A match is stepped by selfplay.hip's loop.
#include "host_common.hpp"

// the line of handle-local game `game`: with alternating colours the games 2j and 2j + 1 share line j
static size_t sp_line_of(const sc_selfplay* sp, int game) {
    return (size_t)((sp->p.match_colours ? game >> 1 : game) % sp->open_lines.n);
}
int sp_opening(const sc_selfplay* sp, int game, const uint16_t** moves) {
    if (sp->open_lines.n <= 0) return 0;
    const size_t i = sp_line_of(sp, game);
    if (moves) *moves = sp->open_moves.data() + sp->open_move_off[i];
    return (int)(sp->open_move_off[i + 1] - sp->open_move_off[i]);
}
const char* sp_opening_fen(const sc_selfplay* sp, int game) {
    if (sp->open_lines.n <= 0 || sp->open_fens.empty()) return nullptr;
    const size_t i = sp_line_of(sp, game);
    return sp->open_fens[i].empty() ? nullptr : sp->open_fens[i].c_str();
}

// what both match forms ask of the rollout and the engines
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
static void match_set_players(sc_selfplay* sp, sc_engine* a, sc_engine* b, uint64_t salt_a, uint64_t salt_b) {
    sp->match = true;
    sp->player[0] = a;
    sp->player[1] = b;
    sp->salt[0] = salt_a;
    sp->salt[1] = salt_b;
}

// Nothing has run on the handle yet: the slots' initial draw (sc_selfplay_create: slot g plays game g) is taken back and made
// again, by the match's start rule and with `lines`
static int sp_redraw_slots(sc_selfplay* sp, const sc::MatchLines& lines) {
    const sc::SpParams& p = sp->p;
    HIPOK(hipMemsetAsync(p.cnt, 0, sizeof(sc::Counters), sp->stream));
    HIPOK(hipMemsetAsync(p.ctl, 0, (size_t)p.n_slots * sizeof(sc::GameCtl), sp->stream));
    HIPOK(hipMemsetAsync(p.thdr, 0, (size_t)p.trace_cap * sizeof(sc::TraceHdr), sp->stream));
    scl::init_slots(p, lines, sp->stream);   // (match_side = 0: the boundary of ply 0)
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(sp->stream));
    return 0;
}

extern "C" {

int sc_selfplay_set_players(sc_selfplay* sp, sc_engine* white, sc_engine* black, uint64_t salt_white, uint64_t salt_black) {
    if (!sp) return fail("null handle");
    if (sp->external) return fail("set_players: the handle plays an outside opponent (sc_selfplay_set_external)");
    if (sp->sim_steps_enqueued != 0) return fail("set_players must precede the first enqueue");
    if (sp->cfg.n_games != sp->cfg.n_slots) return fail("match play needs n_games == n_slots (lockstep plies, no slot recycling)");
    TRY(match_players_check(sp, white, black));
    match_set_players(sp, white, black, salt_white, salt_black);
    return 0;
}

int sc_selfplay_set_match(sc_selfplay* sp, sc_engine* a, sc_engine* b, uint64_t salt_a, uint64_t salt_b, int colours) {
    if (!sp) {
        TRY(use_device(nullptr, 0));
        return fail("null handle");
    }
    if (sp->poisoned) return sp_refuse(sp);
    if (sp->external) return fail("set_match: the handle plays an outside opponent (sc_selfplay_set_external)");
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
    p.match_recycle = 1;
    p.match_colours = (uint8_t)colours;
    TRY(sp_redraw_slots(sp, sp->open_lines));   // (no lines yet)
    match_set_players(sp, a, b, salt_a, salt_b);
    return 0;
}

// The lines are replayed and checked ONCE, here (k_open_lines), into records that stay on the device; a game start copies its line's
// records into the slot (k_match_boundary).  As sc_selfplay_set_match does, the slots are then drawn again, now with the lines.
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
    if (sp->external) return fail("set_openings: opening lines against an outside opponent are not supported (sc_selfplay_set_external)");
    if (!sp->p.match_recycle) return fail("set_openings needs a handle set up by sc_selfplay_set_match");
    if (sp->sim_steps_enqueued != 0) return fail("set_openings must precede the first enqueue");
    if (n_lines < 1 || !move_off) return fail("set_openings: bad argument");
    if (!base_idx) bases = nullptr;   // (base_idx is read only where there are bases)
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
        if (len > 600 || (int64_t)pad + len + 1 > (int64_t)sp->p.hist_cap)
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
    const sc::MatchLines lines{d_tab.p, d_roff.p, n_lines};
    TRY(sp_redraw_slots(sp, lines));   // accepted
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
    return copy_text(fen ? fen : "", buf, cap);
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
    if (!sp->p.match_recycle && !sp->external) return fail("match_tally needs a handle set up by sc_selfplay_set_match");
    TRY(sp_quiesce(sp, true));
    scl::match_tally(sp->p.match_tally(), sp->p.n_slots, sp->d_match_sum, sp->stream);
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(sp->stream));
    static_assert(sizeof(long long) == sizeof(int64_t), "the reduction kernel writes int64");
    HIPOK(hipMemcpy(out, sp->d_match_sum, 8 * sizeof(int64_t), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
