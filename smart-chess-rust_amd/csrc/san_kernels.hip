// san_kernels.hip -- games written as SAN movetext (sc_encode_san_device): the parser that resolves SAN tokens against the
// generated legal moves, and the training rows' dist writer for a played move alone (the reference's ValidationDataset:
// count 1 on the move played, 0 on every other legal move).  Of the encoders it shares position_chain.hpp only.
#include "position_chain.hpp"

#include "launchers.hpp"

namespace sc {

// python-chess's SAN pattern, upper-case pieces only: [NBRQK]?[a-h]?[1-8]?[x-]?[a-h][1-8](=?[NBRQ])?, or a castling word
struct SanTok {
    bool ok;
    int castle;   // 0 no, 1 king side, 2 queen side
    int piece;    // PAWN .. KING
    int file, rank;   // of the origin, -1 = not given
    int to, promo;    // promo in the move encoding (0 none, 2 N, 3 B, 4 R, 5 Q)
};

__device__ __forceinline__ int san_piece(int c) { return c == 'N' ? KNIGHT : c == 'B' ? BISHOP : c == 'R' ? ROOK : c == 'Q' ? QUEEN : c == 'K' ? KING : -1; }
__device__ __forceinline__ constexpr uint64_t san_word(const char* s) {
    uint64_t v = 0;
    for (int k = 0; s[k]; k++) v |= (uint64_t)(unsigned char)s[k] << (8 * k);
    return v;
}

// the token is wave-uniform: scalar code, once per ply
__device__ inline SanTok san_decode(uint64_t t) {
    SanTok d{false, 0, PAWN, -1, -1, 0, 0};
    if (t == san_word("O-O") || t == san_word("0-0")) {
        d.ok = true;
        d.castle = 1;
        return d;
    }
    if (t == san_word("O-O-O") || t == san_word("0-0-0")) {
        d.ok = true;
        d.castle = 2;
        return d;
    }
    if (t >> 56) return d;   // the reserved value, or no token of the tokenizer's
    int n = 0;
    while (n < 7 && ((t >> (8 * n)) & 0xff)) n++;
    if (n < 7 && (t >> (8 * n))) return d;   // characters behind a zero byte
    auto ch = [t](int k) { return (int)((t >> (8 * k)) & 0xff); };
    int i = 0;
    if (n > 0 && san_piece(ch(0)) >= 0) {
        d.piece = san_piece(ch(0));
        i = 1;
    }
    if (n - i >= 1) {
        const int pr = san_piece(ch(n - 1));
        if (pr >= KNIGHT && pr <= QUEEN) {
            d.promo = pr + 1;
            n--;
            if (n - i >= 1 && ch(n - 1) == '=') n--;
        }
    }
    if (n - i < 2) return d;
    const int tf = ch(n - 2) - 'a', tr = ch(n - 1) - '1';
    if (tf < 0 || tf > 7 || tr < 0 || tr > 7) return d;
    d.to = tr * 8 + tf;
    n -= 2;
    if (i < n && ch(i) >= 'a' && ch(i) <= 'h') d.file = ch(i++) - 'a';
    if (i < n && ch(i) >= '1' && ch(i) <= '8') d.rank = ch(i++) - '1';
    if (i < n && (ch(i) == 'x' || ch(i) == '-')) i++;
    d.ok = i == n;
    return d;
}

// does the legal move m of position p answer to the token?  The capture mark and the check marks are not verified
// (python-chess does not either); over-specified disambiguation is accepted.
__device__ __forceinline__ bool san_match(const Position& p, const SanTok& d, move_t m) {
    const int from = mv_from(m), to = mv_to(m), promo = mv_promo(m);
    const int pt = piece_type_at(p, from);
    if (d.castle) {
        const int base = p.turn ? 0 : 56;
        return pt == KING && from == base + 4 && to == base + (d.castle == 1 ? 6 : 2);
    }
    return to == d.to && promo == d.promo && pt == d.piece && (d.file < 0 || (from & 7) == d.file) && (d.rank < 0 || (from >> 3) == d.rank);
}

// ------------------------------------------------------------------ the parser
// One wave per game, the plies one after the other, shaped like k_open_lines: generate the legal moves into LDS, decode the
// ply's token on the scalar unit, match with lane = legal-move index in rounds of 64, ballot and count, play the one move that
// matched on the board (make_move_board: legality needs neither keys nor repetition flags; the encoder's own walk computes
// those).  The next ply's token is loaded before this ply's move generation, so its latency hides under the generation.
// status[g]: 0; -(i + 1): token i names no legal move (any token after mate or stalemate does); 100000 + i: it matches more
// than one; 200000 + i: it is malformed or the reserved value.  The first failing ply wins; the game's moves from that ply on
// are written as 0, which no walk plays.  Claimable draws do not stop the parse (python-chess's read_game goes on too).
__global__ __launch_bounds__(64) void k_san_parse(int n_games, const uint64_t* __restrict__ tokens, const uint32_t* __restrict__ tok_off,
                                                  uint16_t* __restrict__ moves, int32_t* __restrict__ status, Bases bases) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= n_games) return;
    __shared__ move_t s_moves[MAXC];
    const uint32_t p0 = tok_off[g];
    const int nm = (int)(tok_off[g + 1] - p0);
    const uint64_t* tk = tokens + p0;
    uint16_t* out = moves + p0;
    Position cur = chain_start(bases, g, false);
    int st = 0, j = 0;
    uint64_t next = nm > 0 ? tk[0] : 0;
    for (; j < nm; j++) {
        const uint64_t t = uniform(next);
        if (j + 1 < nm) next = tk[j + 1];
        int nl = 0;
        gen_legal_wave(cur, s_moves, lane, nl);
        __syncthreads();
        const SanTok d = san_decode(t);
        int cnt = 0, hit = 0;
        if (d.ok) {
            for (int b = 0; b < nl; b += 64) {
                const int i = b + lane;
                const int m = i < nl ? (int)s_moves[i] : 0;
                const uint64_t bal = __ballot(i < nl && san_match(cur, d, (move_t)m));
                if (bal) {
                    cnt += __popcll(bal);
                    hit = __builtin_amdgcn_readlane(m, uniform((int)__builtin_ctzll(bal)));
                }
            }
        }
        __syncthreads();   // the next generation overwrites s_moves
        if (!d.ok) st = 200000 + j;
        else if (cnt == 0) st = -(j + 1);
        else if (cnt > 1) st = 100000 + j;
        if (st) break;
        if (lane == 0) out[j] = (uint16_t)hit;
        make_move_board(cur, (move_t)hit);
    }
    for (int k = j + lane; k < nm; k += 64) out[k] = 0;
    if (lane == 0) status[g] = st;
}

// ------------------------------------------------------------------ dist of a played move alone
// k_steps_dist (encode_kernels.hip) for children that are the legal moves with count 1 on the played move and 0 elsewhere: the
// same outputs in the same arithmetic -- dist = count / (sum + 1e-5) with sum = 1, the (mirrored) meta in the requested layout,
// whole rows written -- without reading children and without the two checks, which the parser has made.  A ply whose move is
// not among the legal moves (the 0 of a failed game) gets all-zero rows.
__global__ __launch_bounds__(64) void k_san_dist(int n, PlyMoves pm, RowOut o) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= n) return;
    const int nl = pm.n_legal[g];
    const int turn = o.meta_s[(size_t)g * 7];
    const move_t nx = pm.next_mv[g];
    const float share = 1.f / (1.f + 1e-5f);   // count 1 of a sum of 1
    if (o.dist) {
        float4* dz = reinterpret_cast<float4*>(o.dist + (size_t)g * 4672);
        for (int i = lane; i < 4672 / 4; i += 64) dz[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    for (int i = lane; i < MAXC; i += 64) {
        const bool played = i < nl && pm.legal_mv[(size_t)g * MAXC + i] == nx;
        if (played && o.dist) {
            const int idx = move_index(nx, turn);
            if (idx >= 0) o.dist[(size_t)g * 4672 + idx] = share;
        }
        if (o.dist_legal) o.dist_legal[(size_t)g * MAXC + i] = played ? share : 0.f;
    }
    if (o.n_legal && lane == 0) o.n_legal[g] = nl;
    write_meta_row(o, g, lane);
}

}  // namespace sc

namespace scl {
void san_parse(int n_games, const uint64_t* d_tokens, const uint32_t* d_tok_off, uint16_t* d_moves, int32_t* d_status,
               const sc::Bases& bases, hipStream_t s) {
    if (n_games <= 0) return;
    hipLaunchKernelGGL(sc::k_san_parse, dim3(n_games), dim3(64), 0, s, n_games, d_tokens, d_tok_off, d_moves, d_status, bases);
}
void san_dist(int n, const sc::PlyMoves& m, const sc::RowOut& o, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(sc::k_san_dist, dim3(n), dim3(64), 0, s, n, m, o);
}
}  // namespace scl
