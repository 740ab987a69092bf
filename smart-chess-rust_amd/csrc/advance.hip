// advance.hip -- host side of libsc_engine.so: sc_selfplay_advance (include/sc_engine.h), a move played in many slots at once with
// the searched subtree below it kept (advance_kernels.hip).  One small read of the control blocks sizes the kernel's marks -- one
// word per LIVE node of the listed slots, never node_cap x n_slots (an interactive handle's pool has 13 M nodes) --, one launch does
// the work, one copy brings status and counts back.
#include "host_common.hpp"

extern "C" {

int sc_selfplay_advance(sc_selfplay* sp, int n, const int32_t* slots, const uint16_t* moves, int32_t* status, int32_t* kept) {
    if (!sp || n < 0 || (n > 0 && (!slots || !moves))) return fail("bad argument");
    if (sp->poisoned) return sp_refuse(sp);
    if (sp->external) return fail("advance: the plies of an external handle end on the device (sc_selfplay_push_moves plays the opponent's moves)");
    if (sp->cfg.rollout_factor > 0.f) return fail("advance needs a fixed rollout: a rollout_factor budget is chosen when the root is the leaf, which a kept root never is");
    if (n == 0) return 0;
    const sc::SpParams& p = sp->p;
    std::vector<char> seen((size_t)p.n_slots, 0);
    for (int i = 0; i < n; i++) {
        if (slots[i] < 0 || slots[i] >= p.n_slots) return fail("advance: slot " + std::to_string(slots[i]) + " of " + std::to_string(p.n_slots));
        if (seen[(size_t)slots[i]]) return fail("advance: slot " + std::to_string(slots[i]) + " is listed twice");
        seen[(size_t)slots[i]] = 1;
    }
    TRY(sp_quiesce(sp, true));
    // the live node counts: entry i owns marks[off[i] .. off[i + 1])
    std::vector<sc::GameCtl> ctl((size_t)p.n_slots);
    HIPOK(hipMemcpy(ctl.data(), p.ctl, ctl.size() * sizeof(sc::GameCtl), hipMemcpyDeviceToHost));
    std::vector<uint64_t> off((size_t)n + 1, 0);
    for (int i = 0; i < n; i++) {
        const int32_t live = ctl[(size_t)slots[i]].n_nodes;
        off[(size_t)i + 1] = off[(size_t)i] + (uint64_t)std::min(std::max(live, 1), p.node_cap);
    }
    const auto wait = [sp] { return hipStreamSynchronize(sp->stream); };
    TRY(sp->d_adv_marks.grow((size_t)off[(size_t)n], wait));
    const size_t N = (size_t)n;
    const auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_slots = 0, o_moves = o_slots + up(N * 4), o_status = o_moves + up(N * 2), o_kept = o_status + up(N * 4),
                 o_off = o_kept + up(N * 12), bytes = o_off + up((N + 1) * 8);
    TRY(sp->d_adv.grow(bytes, wait));
    char* d = sp->d_adv.p;
    HIPOK(hipMemcpyAsync(d + o_slots, slots, N * 4, hipMemcpyHostToDevice, sp->stream));
    HIPOK(hipMemcpyAsync(d + o_moves, moves, N * 2, hipMemcpyHostToDevice, sp->stream));
    HIPOK(hipMemcpyAsync(d + o_off, off.data(), (N + 1) * 8, hipMemcpyHostToDevice, sp->stream));
    HIPOK(hipMemsetAsync(sp->d_adv_marks.p, 0, (size_t)off[N] * 4, sp->stream));
    scad::AdvanceArgs a{};
    a.n = n;
    a.slots = reinterpret_cast<const int32_t*>(d + o_slots);
    a.moves = reinterpret_cast<const uint16_t*>(d + o_moves);
    a.status = reinterpret_cast<int32_t*>(d + o_status);
    a.kept = reinterpret_cast<int32_t*>(d + o_kept);
    a.scratch = sp->d_adv_marks.p;
    a.off = reinterpret_cast<const uint64_t*>(d + o_off);
    // a game that the move ends is finished under the handle's own rule, as sc_selfplay_push_moves finishes it: a recycled slot
    // goes idle and its boundary kernel takes over, any other slot draws the next game at once
    sc::SpParams q = p;
    if (p.match_recycle) q.total_games = 0;
    scl::advance(q, a, sp->stream);
    HIPOK(hipGetLastError());
    std::vector<int32_t> st(N), kp(N * 3);
    HIPOK(hipMemcpyAsync(st.data(), d + o_status, N * 4, hipMemcpyDeviceToHost, sp->stream));
    HIPOK(hipMemcpyAsync(kp.data(), d + o_kept, N * 12, hipMemcpyDeviceToHost, sp->stream));
    HIPOK(hipStreamSynchronize(sp->stream));
    int refused = 0;
    for (size_t i = 0; i < N; i++) refused += st[i] < 0;
    if (status) std::copy(st.begin(), st.end(), status);
    if (kept) std::copy(kp.begin(), kp.end(), kept);
    return refused;
}

}  // extern "C"
