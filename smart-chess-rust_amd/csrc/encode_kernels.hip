// encode_kernels.hip -- the encoders off the search's path (positions from move lists, training tensors of recorded games) and their
// launchers; of the search they share position_chain.hpp only.  Built with -ffp-contract=off like mcts_kernels.hip (search_select.hpp).
#include "position_chain.hpp"

#include "launchers.hpp"

namespace sc {
// ------------------------------------------------------------------ sc_encode_positions
// One wave per position: replay the move list from the position's start (chain_start), validating every move
// against the legal-move generator, then produce the NN input, the legal moves + action indices
// and outcome(claim_draw=True).  hist scratch: [n][hist_cap] Positions.
__global__ __launch_bounds__(64) void k_encode_positions(GameWalk w, PlyRows rows, int32_t* outcome) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= w.n_games) return;
    int8_t* boards = static_cast<int8_t*>(rows.boards);
    __shared__ __attribute__((aligned(16))) int8_t s_stage[7168];
    __shared__ move_t s_moves[MAXC];
    __shared__ Position s_np;
    Position* hist = w.hist + (size_t)g * w.hist_cap;
    const uint16_t* mv = w.moves + w.move_off[g];
    const int nm = (int)(w.move_off[g + 1] - w.move_off[g]);
    Position cur = chain_start(w.bases, g, true);
    if (lane == 0) hist[0] = cur;
    __syncthreads();
    int status;
    const int played = replay_checked(cur, mv, min(nm, w.hist_cap - 1), hist, s_moves, &s_np, lane, status);
    HistChain hc{hist};
    int n = 0;
    bool in_check = gen_legal_wave(cur, s_moves, lane, n);
    __syncthreads();
    if (rows.legal_mv)
        for (int i = lane; i < n; i += 64) rows.legal_mv[(size_t)g * MAXC + i] = s_moves[i];
    if (rows.legal_idx)
        for (int i = lane; i < n; i += 64) rows.legal_idx[(size_t)g * MAXC + i] = (uint16_t)move_index(s_moves[i], cur.turn);
    if (rows.n_legal && lane == 0) rows.n_legal[g] = n;
    if (boards) {
        __shared__ int32_t s_meta[8];
        __shared__ Position s_hist[8];
        stage_history(hc, played, lane, s_hist);
        __syncthreads();
        encode_wave(s_hist, played < 7 ? played + 1 : 8, lane, s_stage, boards + (size_t)g * 7168, s_meta);
        __syncthreads();
        if (rows.meta && lane < 7) rows.meta[(size_t)g * 7 + lane] = s_meta[lane];
    } else if (rows.meta && lane == 0) {
        int32_t m[7];
        encode_meta(cur, m);
        for (int k = 0; k < 7; k++) rows.meta[(size_t)g * 7 + k] = m[k];
    }
    if (outcome) {
        int winner = -1;
        int term = outcome_claim_draw(hc, played, &winner);
        if (lane == 0) {
            outcome[(size_t)g * 4 + 0] = term;
            outcome[(size_t)g * 4 + 1] = winner;
            outcome[(size_t)g * 4 + 2] = in_check ? 1 : 0;
            outcome[(size_t)g * 4 + 3] = status;
        }
    }
}

// ------------------------------------------------------------------ trace replay for the training-tensor encoder
// sc_encode_steps needs every ply of every game.  Replaying each ply's prefix in its own wave (k_encode_positions) is
// O(plies^2) make_move + move generations per game; here a game is walked ONCE by one wave -- make_move, transposition key,
// repetition flags, one 80-byte record per ply -- and the plies are then encoded in parallel from those records
// (k_encode_plies).  The walk does not validate the moves (that needs a move generation per ply: the per-ply kernel has
// one anyway, and k_steps_dist checks the played move against it); it only refuses moves make_move could not execute
// safely -- no piece of the mover on the from-square, an own piece on the target, a promotion code outside {0, N, B, R, Q}
// or on a non-pawn -- and leaves the position unchanged for those (the ply is then reported as illegal by the per-ply check,
// and the game's later plies are unspecified, include/sc_engine.h).
__global__ __launch_bounds__(64) void k_replay_raw(GameWalk w) {
    // the only sequential part: one wave per game, board updates only (make_move_board: ~10 % of what a full make_move + repetition
    // scan per ply cost when this kernel did everything -- 1.9 us per ply, 194 us for 100-ply games)
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= w.n_games) return;
    Position* hist = w.hist + (size_t)g * w.hist_cap;
    const uint16_t* mv = w.moves + w.move_off[g];
    const int nm = (int)(w.move_off[g + 1] - w.move_off[g]);
    Position cur = chain_start(w.bases, g, false);
    if (lane == 0) hist[0] = cur;
    int mv64 = 0;   // the next 64 moves of the game, one per lane: one load per 64 plies instead of a dependent load per ply
    for (int i = 0; i < nm && i + 1 < w.hist_cap; i++) {
        if ((i & 63) == 0) mv64 = (i + lane < nm) ? (int)mv[i + lane] : 0;
        const move_t m = (move_t)__builtin_amdgcn_readlane(mv64, i & 63);
        const int from = mv_from(m), to = mv_to(m), promo = mv_promo(m);
        const bool ours = (occ_c(cur, cur.turn) & bit(from)) != 0, own_target = (occ_c(cur, cur.turn) & bit(to)) != 0;
        const bool promo_ok = promo == 0 || (promo >= 2 && promo <= 5 && (cur.pcs[PAWN] & bit(from)) != 0);
        if (ours && !own_target && promo_ok && from != to) make_move_board(cur, m);
        if (lane == 0) hist[i + 1] = cur;
    }
}

// one wave per ply, after k_replay_raw: the record's key, and F_IRREV of the move that led to it (python-chess is_irreversible on
// the position before: zeroing, castling rights reduced, or a legal en-passant capture was available)
__global__ __launch_bounds__(64) void k_ply_keys(int n, Position* hist_all, PlyIndex idx, const uint16_t* ply_move) {
    const int q = blockIdx.x, lane = threadIdx.x;
    if (q >= n) return;
    Position* hist = hist_all + idx.hoff[q];
    const int i = (int)idx.plen[q];
    const Position pos = uniform(hist[i]);
    const bool epl = has_legal_ep(pos);
    const bb_t key = position_key_wave(pos, lane, epl);
    uint8_t fl = 0;
    if (i > 0) {
        const Position prev = uniform(hist[i - 1]);
        const move_t m = (move_t)uniform((int)ply_move[q - 1]);   // the game's previous ply is the previous ply of the batch
        fl = (is_zeroing(prev, m) || reduces_castling(prev, m) || has_legal_ep(prev)) ? F_IRREV : 0;
    }
    if (lane == 0) {
        hist[i].key = key;
        hist[i].flags = fl;
    }
}
// ... and, with every key and F_IRREV in place, the repetition flags (planes 12 / 13): is_repetition(2) / is_repetition(3)
__global__ __launch_bounds__(64) void k_ply_rep(int n, Position* hist_all, PlyIndex idx) {
    const int q = blockIdx.x, lane = threadIdx.x;
    if (q >= n) return;
    Position* hist = hist_all + idx.hoff[q];
    const int i = (int)idx.plen[q];
    const HistChain ch{hist};
    const bb_t key0 = uniform(hist[i].key);
    const uint8_t rf = (uint8_t)__builtin_amdgcn_readfirstlane((int)rep_flags_wave(ch, i, key0, lane));
    // (a byte store beside the F_IRREV bit other waves' scans read: that bit does not change here)
    if (lane == 0 && rf) hist[i].flags = (uint8_t)((hist[i].flags & F_IRREV) | rf);
}

// ------------------------------------------------------------------ training tensors
// Per ply of a recorded game: libsmartchess.chess_encode_steps (reference src/lib.rs:46-128), for sc_encode_steps (through
// staging), sc_encode_steps_device and sc_selfplay_encode_traces (straight into the caller's device buffers).  After the walk
// above, one wavefront per ply, two kernels:
//   k_encode_plies<LAYOUT>: legal moves (python-chess order), action indices, planes and meta of the position BEFORE the ply's
//     move, from the game's records.  LAYOUT 0 is the reference's int8 [8][8][112], LAYOUT 1 the trainer's float32 [112][8][8];
//   k_steps_dist: the reference's two panics -- the searched children must be exactly the legal moves, the played move must be
//     legal -- and dist[index(move)] = count / (sum + 1e-5), index by the REAL mover (lib.rs:85-92, 105-113); HBM-bound
//     writer (18.7 KB of dist per ply).  The children come as CSR arrays or as the trace ring's padded rows.
//   apply_mirror: the planes and dist do not change (the stored boards are rotated once at push and once more at view,
//     lib.rs:80-98 + chess.rs:827-842 -- asserted on the oracle's literal restatement); meta becomes that of Board::rotate():
//     [!turn, fullmove + (turn==White), K(opp), Q(opp), K(mover), Q(mover), halfmove].
// Every output but status is optional (nullptr).  A game's status is reduced on the device: k_steps_dist folds each failing
// ply into status[game] by an atomic min, k_status_final turns the result into the codes of include/sc_engine.h.
// per ply q of the games [g0, g0 + ng) (plies ply_off[g0] + [0, n)): its game, its index in the game and the record offset of
// its game in the group's history buffer (group-local: ng * hist_cap records).  From the trace ring (t_move != nullptr) also
// the ply's move and its ring index row * num_steps + ply, so that the replay reads a packed move list.  One thread per ply.
__global__ __launch_bounds__(256) void k_ply_index(PlyGroup gr, PlyIndex idx, RingPlies ring) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= gr.n) return;
    const uint32_t q = gr.ply_off[gr.g0] + (uint32_t)i;
    int lo = gr.g0, hi = gr.g0 + gr.ng - 1;   // the last game whose first ply is <= q (a game without plies shares its offset with the next)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (gr.ply_off[mid] <= q) lo = mid;
        else hi = mid - 1;
    }
    const uint32_t t = q - gr.ply_off[lo];
    idx.hoff[q] = (uint32_t)(lo - gr.g0) * (uint32_t)gr.hist_cap;
    idx.plen[q] = t;
    idx.pgame[q] = (uint32_t)lo;
    if (ring.t_move) {
        const uint32_t s = (uint32_t)ring.rows[lo] * (uint32_t)ring.num_steps + t;
        ring.moves[q] = ring.t_move[s];
        ring.src[q] = s;
    }
}

// hoff[p]: record index of the game's start position, plen[p]: moves played before the ply.  LAYOUT 0: int8 [n][8][8][112] as
// encode_wave writes it; LAYOUT 1: float32 [n][112][8][8] -- lane = square, one plane per store, so each of the 112 stores of
// a ply is one contiguous 256-byte row.  meta (int32, stride 7), legal_mv and n_legal are the call's scratch (k_steps_dist
// reads them); boards and legal_idx are the caller's buffers or nullptr.  Whole rows are written: the entries past n_legal are
// zero (include/sc_engine.h).
template <int LAYOUT>
__global__ __launch_bounds__(64) void k_encode_plies(int n, const Position* hist_all, PlyIndex idx, PlyRows rows) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= n) return;
    __shared__ __attribute__((aligned(16))) int8_t s_stage[7168];
    __shared__ move_t s_moves[MAXC];
    __shared__ int32_t s_meta[8];
    __shared__ Position s_hist[8];
    const HistChain hc{hist_all + idx.hoff[g]};
    const int played = (int)idx.plen[g];
    stage_history(hc, played, lane, s_hist);
    __syncthreads();
    const Position cur = s_hist[0];
    int nl = 0;
    gen_legal_wave(cur, s_moves, lane, nl);
    __syncthreads();
    for (int i = lane; i < MAXC; i += 64) {
        rows.legal_mv[(size_t)g * MAXC + i] = i < nl ? s_moves[i] : (move_t)0;
        if (rows.legal_idx) rows.legal_idx[(size_t)g * MAXC + i] = i < nl ? (uint16_t)move_index(s_moves[i], cur.turn) : (uint16_t)0;
    }
    if (lane == 0) rows.n_legal[g] = nl;
    int8_t* out8 = (LAYOUT == 0 && rows.boards) ? static_cast<int8_t*>(rows.boards) + (size_t)g * 7168 : nullptr;
    encode_wave(s_hist, played < 7 ? played + 1 : 8, lane, s_stage, out8, s_meta);
    if (LAYOUT == 1 && rows.boards) {
        // this lane's own 112 plane bytes (written by this lane above), widened to float, plane by plane
        const uint4* cell16 = reinterpret_cast<const uint4*>(s_stage + lane * 112);
        uint32_t w[28];
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const uint4 v = cell16[k];
            w[4 * k] = v.x;
            w[4 * k + 1] = v.y;
            w[4 * k + 2] = v.z;
            w[4 * k + 3] = v.w;
        }
        float* o = static_cast<float*>(rows.boards) + (size_t)g * 7168 + lane;
#pragma unroll
        for (int c = 0; c < 112; c++) o[c * 64] = (float)(int8_t)((w[c >> 2] >> (8 * (c & 3))) & 0xffu);
    }
    __syncthreads();
    if (lane < 7) rows.meta[(size_t)g * 7 + lane] = s_meta[lane];
}

// Children come either as CSR or as the trace ring's padded rows (sc::Children).  Writes the (mirrored) meta in the
// requested layout, the dense dist row, the legal-move row dist_legal[q][i] = share of legal move i (0 past n_legal), n_legal,
// and folds the ply's failure into status[game] with an atomic min over the key 2 * ply + kind (kind 0: children are not the
// legal moves, kind 1: the played move is illegal) -- the first failing ply wins, a children mismatch beats an illegal move
// at the same ply (the reference's precedence); k_status_final turns the keys into sc_encode_steps's codes.
__global__ __launch_bounds__(64) void k_steps_dist(int n, PlyMoves pm, Children ch, PlyIndex idx, RowOut o, int32_t* status) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= n) return;
    __shared__ move_t s_lm[MAXC];
    __shared__ int s_hit[MAXC];
    __shared__ uint32_t s_cn[MAXC];
    const int nl = pm.n_legal[g];
    size_t c0;
    int nc;
    if (ch.src) {
        const uint32_t s = ch.src[g];
        c0 = (size_t)s * MAXC;
        nc = ch.nchild[s];
        nc = nc < 0 ? 0 : nc > MAXC ? MAXC : nc;
    } else {
        c0 = ch.off[g];
        nc = (int)(ch.off[g + 1] - ch.off[g]);
    }
    const int turn = o.meta_s[(size_t)g * 7];
    if (o.dist) {
        float4* dz = reinterpret_cast<float4*>(o.dist + (size_t)g * 4672);
        for (int i = lane; i < 4672 / 4; i += 64) dz[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int i = lane; i < MAXC; i += 64) {
        s_lm[i] = i < nl ? pm.legal_mv[(size_t)g * MAXC + i] : (move_t)0;
        s_hit[i] = 0;
        s_cn[i] = 0;
    }
    __syncthreads();
    const move_t nx = pm.next_mv[g];
    const bool any_next = legal_has_move(s_lm, nl, nx, lane);
    int bad = 0;
    uint32_t sum = 0;
    for (int i = lane; i < nc; i += 64) {
        const move_t m = ch.mv[c0 + i];
        int k = -1;
        for (int j = 0; j < nl; j++)
            if (s_lm[j] == m) k = j;
        if (k < 0) bad = 1;
        else {
            s_hit[k] = 1;     // benign same-value race between duplicates
            s_cn[k] = ch.n[c0 + i];
        }
        sum += ch.n[c0 + i];
    }
    __syncthreads();
    for (int i = lane; i < nl; i += 64) bad |= s_hit[i] ? 0 : 1;   // with nc == nl this also catches duplicate children
    bad |= (nc != nl) ? 1 : 0;
    for (int sh = 32; sh > 0; sh >>= 1) sum += __shfl_xor(sum, sh, 64);   // u32 wrap-around, as the reference's u32 sum in release mode
    const float den = (float)sum + 1e-5f;
    if (o.dist)
        for (int i = lane; i < nc; i += 64) {
            const int ai = move_index(ch.mv[c0 + i], turn);
            if (ai >= 0) o.dist[(size_t)g * 4672 + ai] = (float)ch.n[c0 + i] / den;
        }
    if (o.dist_legal)
        for (int i = lane; i < MAXC; i += 64) o.dist_legal[(size_t)g * MAXC + i] = (i < nl && s_hit[i]) ? (float)s_cn[i] / den : 0.f;
    const bool any_bad = __ballot(bad) != 0;
    if (lane == 0) {
        if (any_bad || !any_next) atomicMin(&status[idx.pgame[g]], (int32_t)(2 * idx.plen[g] + (any_bad ? 0 : 1)));
        if (o.n_legal) o.n_legal[g] = nl;
    }
    write_meta_row(o, g, lane);
}

// status keys (2 * ply + kind, STATUS_NONE when no ply failed) -> 0 / 1000 + ply / -(ply + 1)
__global__ __launch_bounds__(256) void k_status_final(int n, int32_t* status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t v = status[i];
    status[i] = v == STATUS_NONE ? 0 : (v & 1) ? -((v >> 1) + 1) : 1000 + (v >> 1);
}

}  // namespace sc

namespace scl {
void encode_positions(const sc::GameWalk& w, const sc::PlyRows& rows, int32_t* outcome, hipStream_t s) {
    hipLaunchKernelGGL(sc::k_encode_positions, dim3(w.n_games), dim3(64), 0, s, w, rows, outcome);
}
void ply_index(const sc::PlyGroup& g, const sc::PlyIndex& idx, const sc::RingPlies& ring, hipStream_t s) {
    if (g.n <= 0) return;
    hipLaunchKernelGGL(sc::k_ply_index, dim3((g.n + 255) / 256), dim3(256), 0, s, g, idx, ring);
}
void replay_walk(const sc::GameWalk& w, hipStream_t s) {
    if (w.n_games <= 0) return;
    hipLaunchKernelGGL(sc::k_replay_raw, dim3(w.n_games), dim3(64), 0, s, w);
}
void replay_games(const sc::GameWalk& w, int n_plies, const sc::PlyIndex& idx, const uint16_t* d_ply_moves, hipStream_t s) {
    if (w.n_games <= 0 || n_plies <= 0) return;
    replay_walk(w, s);
    hipLaunchKernelGGL(sc::k_ply_keys, dim3(n_plies), dim3(64), 0, s, n_plies, w.hist, idx, d_ply_moves);
    hipLaunchKernelGGL(sc::k_ply_rep, dim3(n_plies), dim3(64), 0, s, n_plies, w.hist, idx);
}
void encode_plies(int layout, int n, const sc::Position* d_hist, const sc::PlyIndex& idx, const sc::PlyRows& rows, hipStream_t s) {
    if (n <= 0) return;
    if (layout == 1) hipLaunchKernelGGL(sc::k_encode_plies<1>, dim3(n), dim3(64), 0, s, n, d_hist, idx, rows);
    else hipLaunchKernelGGL(sc::k_encode_plies<0>, dim3(n), dim3(64), 0, s, n, d_hist, idx, rows);
}
void steps_dist(int n, const sc::PlyMoves& m, const sc::Children& c, const sc::PlyIndex& idx, const sc::RowOut& o, int32_t* status,
                hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(sc::k_steps_dist, dim3(n), dim3(64), 0, s, n, m, c, idx, o, status);
}
void status_final(int n, int32_t* status, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(sc::k_status_final, dim3((n + 255) / 256), dim3(256), 0, s, n, status);
}
}  // namespace scl
