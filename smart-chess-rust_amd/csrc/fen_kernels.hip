// fen_kernels.hip -- positions given as FEN: the raw fields the host's reader leaves (fen_text.cpp) -> validated records in the
// form every kernel of the library expects, and the en-passant bit of python-chess's Board.fen().  Off the search's path: of the
// search these kernels share position_chain.hpp only.
#include "position_chain.hpp"

#include "../../include/sc_engine.h"
#include "launchers.hpp"

namespace sc {

static_assert(sizeof(sc_fen_fields) == 88, "sc_fen_fields layout");

// python-chess Board._valid_ep_square(): the square survives only on the right rank for the side to move, with an enemy pawn in
// front of it and with itself and the square behind it empty
__device__ inline int valid_ep_square(const Position& p, int ep) {
    if (ep < 0 || ep > 63) return -1;
    const bb_t b = bit(ep), occ = all_occ(p);
    const bb_t pawn = p.turn ? b >> 8 : b << 8, behind = p.turn ? b << 8 : b >> 8;
    if ((ep >> 3) != (p.turn ? 5 : 2)) return -1;
    if (!(p.pcs[PAWN] & occ_c(p, !p.turn) & pawn)) return -1;
    if (occ & (b | behind)) return -1;
    return ep;
}
// promoted pieces a colour must have made to own these men: every knight, bishop and rook past the second, every queen past the first
__device__ inline int promoted_men(const Position& p, bb_t own) {
    const int n = popcnt(p.pcs[KNIGHT] & own) - 2, b = popcnt(p.pcs[BISHOP] & own) - 2, r = popcnt(p.pcs[ROOK] & own) - 2;
    const int q = popcnt(p.pcs[QUEEN] & own) - 1;
    return (n > 0 ? n : 0) + (b > 0 ? b : 0) + (r > 0 ? r : 0) + (q > 0 ? q : 0);
}

// The checks of include/sc_engine.h in their order; 0 when the move generator may see the position.  What the generator (gen_legal,
// gen_legal_wave) and its callers assume of their input, and the check that grants it:
//   one piece type per occupied square, occupancy = the union of the types (piece_type_at, xor_pcs)            -6
//   msb() of each side's king bitboard IS the king (king scans, castling, pins)                                -1
//   no pawn on the last ranks (a push from there would leave the board: square index + 8 > 63)                 -2
//   the side to move cannot capture the king (the search's trees never hold such a node)                       -3
//   at most 218 moves, every category total of the packed suffix scan below 256, 4672-wide action indices:
//   true of every position a game can reach, i.e. at most 16 men and 8 pawns a side, promotions paid by pawns  -4
//   evasions look at one or two checkers                                                                       -5
__device__ inline int playable_checks(const Position& p) {
    const bb_t occ = all_occ(p);
    bb_t seen = 0, twice = 0;
#pragma unroll
    for (int t = 0; t < 6; t++) {
        twice |= seen & p.pcs[t];
        seen |= p.pcs[t];
    }
    if (twice || seen != occ || (p.occ[0] & p.occ[1])) return -6;
    const bb_t wk = p.pcs[KING] & p.occ[WHITE], bk = p.pcs[KING] & p.occ[BLACK];
    if (popcnt(wk) != 1 || popcnt(bk) != 1) return -1;
    if (p.pcs[PAWN] & (RANK_1 | RANK_8)) return -2;
    const int us = p.turn;
    const int our_king = msb(us ? wk : bk), their_king = msb(us ? bk : wk);
    if (attackers_mask(p, us, their_king, occ)) return -3;
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const bb_t own = occ_c(p, c);
        const int pawns = popcnt(p.pcs[PAWN] & own);
        if (popcnt(own) > 16 || pawns > 8 || promoted_men(p, own) > 8 - pawns) return -4;
    }
    if (popcnt(attackers_mask(p, !us, our_king, occ)) > 2) return -5;
    return 0;
}

// One wave per position, shaped like k_open_lines.  syntax[g] < 0: the host's reader refused the text; its code is the status.
__global__ __launch_bounds__(64) void k_fen_positions(int n, const sc_fen_fields* __restrict__ fields, const int32_t* __restrict__ syntax,
                                                      Position* __restrict__ out, int32_t* __restrict__ status) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= n) return;
    __shared__ move_t s_moves[MAXC];
    Position start;
    set_startpos(start);
    start.key = position_key(start);
    int st = uniform(syntax[g]);
    Position p = start;
    if (st == 0) {
        const sc_fen_fields& f = fields[g];
#pragma unroll
        for (int t = 0; t < 6; t++) p.pcs[t] = uniform((bb_t)f.pcs[t]);
        p.occ[0] = uniform((bb_t)f.occ[0]);
        p.occ[1] = uniform((bb_t)f.occ[1]);
        p.turn = (uint8_t)(uniform(f.turn) ? WHITE : BLACK);
        p.halfmove = (uint16_t)uniform(f.halfmove);
        p.fullmove = (uint16_t)uniform(f.fullmove);
        p.flags = 0;
        // clean_castling_rights (standard chess): a right needs its king and its rook at home
        const bb_t wk = p.pcs[KING] & p.occ[WHITE], bk = p.pcs[KING] & p.occ[BLACK];
        const bb_t wr = p.pcs[ROOK] & p.occ[WHITE], br = p.pcs[ROOK] & p.occ[BLACK];
        int cr = uniform(f.castling) & 15;
        if (!(wk & bit(4))) cr &= ~3;
        if (!(bk & bit(60))) cr &= ~12;
        if (!(wr & bit(7))) cr &= ~1;
        if (!(wr & bit(0))) cr &= ~2;
        if (!(br & bit(63))) cr &= ~4;
        if (!(br & bit(56))) cr &= ~8;
        p.castling = (uint8_t)cr;
        p.ep = (int8_t)valid_ep_square(p, uniform(f.ep));
        st = playable_checks(p);
        if (st == 0) p.key = position_key(p);
        else p = start;
    }
    if (lane == 0) out[g] = p;
    __threadfence_block();
    __syncthreads();
    if (st == 0) {
        int nl = 0, winner = -1;
        gen_legal_wave(p, s_moves, lane, nl);
        __syncthreads();
        const HistChain hc{out + g};
        if (nl == 0 || outcome_claim_draw(hc, 0, &winner) != T_NONE) st = 1;
    }
    if (lane == 0) status[g] = st;
}

// python-chess prints the ep square of a FEN only if a legal en-passant capture exists: one lane per record
__global__ __launch_bounds__(64) void k_fen_ep_legal(int n, const Position* __restrict__ rec, int32_t* __restrict__ ep_legal) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Position p = rec[i];
    ep_legal[i] = (p.ep >= 0 && has_legal_ep(p)) ? 1 : 0;
}

}  // namespace sc

namespace scl {
void fen_positions(int n, const sc_fen_fields* d_fields, const int32_t* d_syntax, sc::Position* d_out, int32_t* d_status, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(sc::k_fen_positions, dim3(n), dim3(64), 0, s, n, d_fields, d_syntax, d_out, d_status);
}
void fen_ep_legal(int n, const sc::Position* d_rec, int32_t* d_ep_legal, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(sc::k_fen_ep_legal, dim3((n + 63) / 64), dim3(64), 0, s, n, d_rec, d_ep_legal);
}
}  // namespace scl
