// san_write_kernels.hip -- moves written as SAN (sc_moves_to_san_device): the inverse of san_kernels.hip's parser.  The writer
// knows every move up front, so nothing here is a chain: the encoder's walk (k_replay_raw, encode_kernels.hip) leaves one record
// per ply, and every ply is then rendered by its own wavefront.  Of the encoders it shares position_chain.hpp only.
#include "position_chain.hpp"

#include "launchers.hpp"

namespace sc {

// ------------------------------------------------------------------ the writer
// One wave per ply q of the batch.  Record i = plen[q] of the ply's game is the position before the move, record i + 1 the one
// after it (the walk has made every move a legal ply needs; the last ply's record nm is written too).  Generate the legal moves
// of record i into LDS, look for the played move and for its rivals with lane = legal-move index in rounds of 64 -- a rival goes
// to the same square with the same kind of piece from another square -- and apply python-chess's rule
// (Board._algebraic_without_suffix): no rival, nothing; a rival on the origin's rank, the file letter; a rival on the origin's
// file, the rank digit; rivals on neither, the file letter.  Pawns have no rivals: the origin file when they capture.  Since only
// LEGAL moves are rivals, a pinned twin does not count.  The suffix comes from a second generation, of record i + 1, in the same
// LDS buffer: in check without a move '#', in check '+', else nothing (stalemate has no mark).
// The token (sc_san_tokenize's format, character k in byte k, the suffix included: at most 7 characters) is wave-uniform and
// built on the scalar unit; lane 0 stores it.  A move that is not legal stores 0 and folds the key 2 * ply + 1 into status[game]
// by an atomic min (k_steps_dist's key of an illegal move: k_status_final turns it into -(ply + 1), the first failing ply wins).
__global__ __launch_bounds__(64) void k_san_write(int n, const Position* __restrict__ hist_all, PlyIndex idx,
                                                  const uint16_t* __restrict__ ply_move, uint64_t* __restrict__ tokens,
                                                  int32_t* __restrict__ status) {
    const int q = blockIdx.x, lane = threadIdx.x;
    if (q >= n) return;
    __shared__ move_t s_moves[MAXC];
    const Position* hist = hist_all + uniform((int)idx.hoff[q]);
    const int i = uniform((int)idx.plen[q]);
    const Position pos = uniform(hist[i]);
    const move_t m = (move_t)uniform((int)ply_move[q]);
    const int from = mv_from(m), to = mv_to(m), promo = mv_promo(m);
    const int pt = piece_type_at(pos, from);
    int nl = 0;
    gen_legal_wave(pos, s_moves, lane, nl);
    __syncthreads();
    uint64_t legal = 0, rival = 0, on_rank = 0, on_file = 0;
    for (int b = 0; b < nl; b += 64) {
        const int k = b + lane;
        const move_t lm = k < nl ? s_moves[k] : (move_t)0;
        const int lf = mv_from(lm);
        const bool r = k < nl && mv_to(lm) == to && lf != from && piece_type_at(pos, lf) == pt;
        legal |= __ballot(k < nl && lm == m);
        rival |= __ballot(r);
        on_rank |= __ballot(r && (lf >> 3) == (from >> 3));
        on_file |= __ballot(r && (lf & 7) == (from & 7));
    }
    __syncthreads();   // the next generation overwrites s_moves
    if (!legal) {
        if (lane == 0) {
            tokens[q] = 0;
            atomicMin(&status[idx.pgame[q]], (int32_t)(2 * i + 1));
        }
        return;
    }
    uint64_t tok = 0;
    int len = 0;
    auto put = [&tok, &len](int c) {
        tok |= (uint64_t)(unsigned)c << (8 * len);
        len++;
    };
    if (pt == KING && (from & 7) == 4 && ((to & 7) == 6 || (to & 7) == 2)) {   // (a king steps one file at most)
        put('O');
        put('-');
        put('O');
        if ((to & 7) == 2) {
            put('-');
            put('O');
        }
    } else {
        const bool capture = (all_occ(pos) & bit(to)) != 0 || (pt == PAWN && (from & 7) != (to & 7));   // ... en passant
        if (pt == PAWN) {
            if (capture) put('a' + (from & 7));
        } else {
            put("?NBRQK"[pt]);
            if (rival) {
                if (on_rank || !on_file) put('a' + (from & 7));
                if (on_file) put('1' + (from >> 3));
            }
        }
        if (capture) put('x');
        put('a' + (to & 7));
        put('1' + (to >> 3));
        if (promo) {
            put('=');
            put("??NBRQ??"[promo]);
        }
    }
    const Position after = uniform(hist[i + 1]);
    int n_after = 0;
    const bool check = gen_legal_wave(after, s_moves, lane, n_after);
    if (check) put(n_after == 0 ? '#' : '+');
    if (lane == 0) tokens[q] = tok;
}

// one thread per ply, behind k_san_write and in front of k_status_final: a game's tokens from its first failing ply on are 0
// (the walk went on from a position the game never had: what the writer made of the later plies means nothing)
__global__ __launch_bounds__(256) void k_san_clip(int n, PlyIndex idx, const int32_t* __restrict__ status, uint64_t* __restrict__ tokens) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const int32_t key = status[idx.pgame[q]];
    if (key != STATUS_NONE && (int32_t)idx.plen[q] >= (key >> 1)) tokens[q] = 0;
}

}  // namespace sc

namespace scl {
void san_write(int n, const sc::Position* d_hist, const sc::PlyIndex& idx, const uint16_t* d_ply_moves, uint64_t* d_tokens,
               int32_t* d_status, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(sc::k_san_write, dim3(n), dim3(64), 0, s, n, d_hist, idx, d_ply_moves, d_tokens, d_status);
}
void san_clip(int n, const sc::PlyIndex& idx, const int32_t* d_status, uint64_t* d_tokens, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(sc::k_san_clip, dim3((n + 255) / 256), dim3(256), 0, s, n, idx, d_status, d_tokens);
}
}  // namespace scl
