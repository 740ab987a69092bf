// merge_types.hpp -- kernel argument block and workspace layout of the position merge (merge_kernels.hip), shared by host code and
// kernels.  Included through launchers.hpp, whose scl::SCAN_TILE sizes the scan's region.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace scmg {

constexpr int CELLS = 7168;      // board bytes per row: 448 16-byte chunks, 7 per lane
constexpr int META = 7;          // int32 per row
constexpr int LEGAL_ROW = 224;   // SC_MAX_MOVES
constexpr int MAX_LEGAL = 218;
constexpr int MAX_IN = 1 << 30;  // positions of one call (the table's slot numbers and the sort's keys stay below 2^31)

enum : int32_t { ST_OK = 0, ST_BAD_LEGAL = 1, ST_OUTSIDE = 2 };   // state[p]: same-sample candidate / n_legal outside 0..218 / row outside

// The regions of the caller's workspace, byte offsets from its (256-byte aligned) start.  Every region is a multiple of 256 bytes.
struct Workspace {
    uint32_t slots;     // the table: a power of two, >= 2 n_in
    size_t key;         // uint64 [n_in][2]   the masked key of position p
    size_t state;       // int32 [n_in]       ST_*
    size_t slot_of;     // int32 [n_in]       the table slot of p's key; after k_verify: the head p is merged into (p itself: a head)
    size_t flag;        // int32 [n_in]       1: p is the head of a group
    size_t gid;         // int32 [n_in]       exclusive scan of flag
    size_t tile_sum;    // int32 [tiles]      the scan's tile totals, then their exclusive scan
    size_t grp;         // uint32 [n_in]      the group of p, n_in for a position in no group: the sort's keys
    size_t pos;         // int32 [n_in]       p: the sort's values
    size_t grp_sorted;  // uint32 [n_in]
    size_t members;     // int32 [n_in]       positions by (group, position)
    size_t seg;         // int32 [n_in + 1]   where group j starts in members
    size_t aux;         // int32 [8]          [0..3] the call's counts, [4] positions in no group
    size_t slot_rep;    // int32 [slots]      the position that claimed the slot (-1: free): its key is the slot's key
    size_t slot_head;   // int32 [slots]      the smallest position with the slot's key
    size_t sort_tmp;    // the radix sort's own scratch
    size_t sort_bytes;
    size_t bytes;
};

inline Workspace workspace(int n_in) {
    Workspace w{};
    const size_t n = n_in > 0 ? (size_t)n_in : 1;
    uint32_t slots = 64;
    while (slots < 2 * n) slots *= 2;
    w.slots = slots;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t o = at;
        at += (bytes + 255) & ~(size_t)255;
        return o;
    };
    w.key = take(n * 16);
    w.state = take(n * 4);
    w.slot_of = take(n * 4);
    w.flag = take(n * 4);
    w.gid = take(n * 4);
    w.tile_sum = take(((n + scl::SCAN_TILE - 1) / scl::SCAN_TILE) * 4);
    w.grp = take(n * 4);
    w.pos = take(n * 4);
    w.grp_sorted = take(n * 4);
    w.members = take(n * 4);
    w.seg = take((n + 1) * 4);
    w.aux = take(32);
    w.slot_rep = take((size_t)slots * 4);
    w.slot_head = take((size_t)slots * 4);
    // the sort of 32-bit keys with 32-bit values: a second copy of both and one 32-bit counter per digit and block of >= 256
    // items at the most (12 n) -- checked against what the sort asks for when it is enqueued
    w.sort_bytes = 32 * n + ((size_t)1 << 20);
    w.sort_tmp = take(w.sort_bytes);
    w.bytes = at + 256;   // room to align the caller's pointer
    return w;
}

// sc_merge_positions (include/sc_engine.h)
struct MergeArgs {
    int n_src;
    int n_in;
    int key_bits;
    const int32_t* rows;         // [n_in] or null: position p is row p
    const int8_t* boards;        // [n_src][8][8][112]
    const int32_t* meta;         // [n_src][7]
    const float* dist_legal;     // [n_src][224]
    const uint16_t* legal_idx;   // [n_src][224]
    const int32_t* n_legal;      // [n_src]
    const float* outcome;        // [n_src]
    char* ws;                    // the workspace, aligned
    int8_t* out_boards;          // [groups][8][8][112], or null (as every output)
    int32_t* out_meta;
    float* out_dist_legal;
    uint16_t* out_legal_idx;
    int32_t* out_n_legal;
    float* out_outcome;
    int32_t* out_count;
    int32_t* out_first;
    int32_t* group_of;           // [n_in]
    int32_t* counts;             // [4], or null
};

}  // namespace scmg
