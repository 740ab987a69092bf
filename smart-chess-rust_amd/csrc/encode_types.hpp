// encode_types.hpp -- kernel argument blocks of the encoders of recorded games (encode_kernels.hip, san_kernels.hip,
// san_write_kernels.hip, k_open_lines), shared by host code and kernels.  Every pointer is device memory.
#pragma once
#include "chess_rules.hpp"

namespace sc {

// the status key (2 * ply + kind, folded by atomic min) of a game without a failing ply, and the byte whose fill leaves it
constexpr int32_t STATUS_NONE = 0x7f7f7f7f;
constexpr int STATUS_FILL_BYTE = 0x7f;

// the bases of a call (rec == nullptr: none): game g starts from record idx[g] of rec (fen_kernels.hip) where that is >= 0
struct Bases {
    const Position* rec;
    const int32_t* idx;   // [games]
    Bases from(int g0) const { return {rec, rec ? idx + g0 : nullptr}; }   // ... of the games from g0 on
};

// the games a walk replays: game g plays moves[move_off[g] .. move_off[g + 1]) into the records hist[g * hist_cap ..]
struct GameWalk {
    int n_games;
    const uint16_t* moves;
    const uint32_t* move_off;   // [n_games + 1]
    Position* hist;
    int hist_cap;
    Bases bases;
};

// the per-ply index of a batch (k_ply_index): record offset of the ply's game in its group, moves played before the ply, its game
struct PlyIndex {
    uint32_t *hoff, *plen, *pgame;
    PlyIndex from(size_t q) const { return {hoff + q, plen + q, pgame + q}; }   // ... of the plies from q on
};

// the plies k_ply_index numbers: the n plies of the games [g0, g0 + ng), whose records are hist_cap apart
struct PlyGroup {
    int n, g0, ng;
    const uint32_t* ply_off;   // of the batch
    int hist_cap;
};
// ... and, from the trace ring (t_move != nullptr), the ply's move and ring index rows[game] * num_steps + ply
struct RingPlies {
    const int32_t* rows;
    int num_steps;
    const uint16_t* t_move;
    uint16_t* moves;   // [plies of the batch]
    uint32_t* src;
};

// what k_encode_plies writes per ply: boards and legal_idx are the caller's or null, the others the call's scratch
struct PlyRows {
    void* boards;
    int32_t* meta;
    uint16_t *legal_mv, *legal_idx;
    int32_t* n_legal;
};
// a ply's legal moves (k_encode_plies) and the move played
struct PlyMoves {
    const uint16_t* legal_mv;
    const int32_t* n_legal;
    const uint16_t* next_mv;
};

// a ply's children: CSR (off[q] .. off[q + 1] into mv / n), or with src the trace ring's rows (row src[q] of MAXC, nchild[src[q]] of them)
struct Children {
    const uint16_t* mv;
    const uint32_t *n, *off, *src;
    const int32_t* nchild;
    Children from(size_t q) const { return {mv, n, off ? off + q : off, src ? src + q : src, nchild}; }   // ... of the plies from q on
};

// the rows k_steps_dist and k_san_dist write per ply, each or null (meta: of meta_s, rotated with apply_mirror; float32 in layout 1)
struct RowOut {
    int apply_mirror;
    const int32_t* meta_s;   // k_encode_plies's meta rows
    int layout;
    void* meta;
    float *dist, *dist_legal;
    int32_t* n_legal;
};

}  // namespace sc
