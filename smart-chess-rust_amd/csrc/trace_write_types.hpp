// trace_write_types.hpp -- kernel argument blocks of the trace-file writer (trace_write_kernels.hip), shared by host code and
// kernels.  Every pointer is device memory.
//
// The text of a call is a sequence of SEGMENTS: for every game its head (up to "steps": and the opening bracket), its plies, its
// tail (the closing bracket, "fen", "opening", the closing brace).  Heads and tails are FRAMES: the host builds their text.
#pragma once
#include <stdint.h>

namespace sctw {

constexpr int ROUND = 64;           // children formatted at a time, one per lane
constexpr int MAX_CHILDREN = 224;   // SC_MAX_MOVES: four rounds at most
constexpr int STAGE_BYTES = 9216;   // LDS of a writer workgroup: 15 bytes of alignment, a step's head (65 at most), 64 children of
                                    // 134 bytes at most, a step's tail (17)
constexpr uint32_t LAST_PLY = 0x80000000u;   // Plies::src: the last ply of its game (no comma behind it)

// the plies of the call's games, one after another
struct Plies {
    uint32_t n;
    const uint32_t* src;   // [n]: the step the ply is read from (an index into Steps' arrays), | LAST_PLY
    const uint32_t* seg;   // [n]: its place in the segment sequence
};
// where the steps are, described like EncodeSrc.  Packed arrays (child_off set): the children of step s are
// [child_off[s], child_off[s + 1]).  The trace ring in place (n_child set): step s = row * num_steps + ply, its children
// s * 224 + [0, n_child[s]).  Q and uct are read as bit patterns.
struct Steps {
    const uint16_t* move;
    const uint32_t* q;
    const uint32_t* child_off;
    const int32_t* n_child;
    const uint16_t* child_move;
    const int32_t* child_n;
    const uint32_t* child_q;
    const uint32_t* child_u;
};
// the frames' text, one after another in blob: frame f is blob[off[f] .. off[f + 1]) and segment seg[f]
struct Frames {
    uint32_t n;
    const char* blob;
    const uint32_t* off;   // [n + 1]
    const uint32_t* seg;   // [n]
};
// the emitting pass of a group of games: seg_off holds the exclusive scan of the group's segment lengths (so the sizes are
// below 2^32), text is the group's buffer, 16-byte aligned
struct Out {
    const uint32_t* seg_off;
    char* text;
};

}  // namespace sctw
