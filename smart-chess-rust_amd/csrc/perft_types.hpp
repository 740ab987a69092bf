// perft_types.hpp -- the node record and the kernel argument blocks of perft on the device (perft_kernels.hip, perft.hip), shared
// by host code and kernels.  Every pointer is device memory; every capacity is in elements of its buffer.
#pragma once
#include "encode_types.hpp"

namespace scpf {

constexpr int ROW = sc::MAX_MOVES;        // a divide row (SC_MAX_MOVES)
constexpr int KINDS = 8;                  // a kinds row: SC_PERFT_* and one reserved slot
constexpr uint32_t DEAD = 0xffffffffu;    // Node::root of a refused entry: it has no children and counts nothing
constexpr uint32_t NO_MOVE = 255;         // the move byte of Node::root at level 0: the root itself, no move yet (a row has 224)
constexpr int MAX_ENTRIES = (1 << 24) - 1;   // entry << 8 | move is one 32-bit number, and DEAD is none of them
constexpr int ATTR_RUN = 16;              // consecutive nodes per thread of k_perft_attribute: 4 096 per workgroup

// A frontier node: the board half of sc::Position -- no key, no clocks, no flags: a generation reads none of them and
// make_move<false> writes none that matter -- and the root move it descends from.  72 bytes
struct Node {
    uint64_t pcs[6];
    uint64_t occ[2];
    uint8_t turn, castling;
    int8_t ep;
    uint8_t pad;
    uint32_t root;   // entry << 8 | index of the entry's move (NO_MOVE at level 0); DEAD: a refused entry
};
static_assert(sizeof(Node) == 72, "Node layout");

// what went wrong inside a kernel: a count that does not match its scan, an index past its buffer.  Nothing is stored through
// such an index; the host turns a non-zero word into an error return
enum { ERR_SLOT = 1, ERR_COUNT = 2, ERR_ENTRY = 4 };

// the entries [e0, e0 + n) of a call: replayed into level 0, slot = entry - e0
struct RootArgs {
    int e0, n;
    const uint16_t* moves;
    const uint32_t* move_off;   // [entries + 1] or null: no entry has moves
    sc::Bases bases;            // idx [entries]
    Node* out;                  // [cap] or null (depth 0: only the status is wanted)
    uint32_t cap;
    int32_t* status;            // [entries]
    int32_t* n_div;             // [entries] or null
    uint16_t* div_moves;        // [entries][ROW] or null
    uint32_t* err;
};

// the nodes [first, first + n) of a level buffer
struct Level {
    const Node* nodes;
    uint32_t first, n;
};

// children of a level's nodes into the next level: node i's go to off[first + i] - base ..., in generator order
struct ExpandArgs {
    Level lv;
    const uint32_t* off;   // [lv's capacity + 1]: the exclusive scan of the counts, the total behind it
    uint32_t base;         // off[first] (the piece's first child is slot 0)
    Node* out;
    uint32_t cap;
    int from_roots;        // level 0 -> 1: child k of an entry gets the move byte k
    uint32_t* err;
};

// the last level: what each node adds, and where the sums go
struct LeafOut {
    uint32_t* cnt;      // [lv.n]: legal moves of the node
    uint32_t* kinds;    // [lv.n][2] or null: captures | ep << 8 | castles << 16 | promotions << 24, then checks | mates << 8
};
struct Totals {
    int n_entries;
    unsigned long long* nodes;       // [entries]
    unsigned long long* kinds;       // [entries][KINDS] or null
    unsigned long long* div_nodes;   // [entries][ROW] or null
    uint32_t* err;
};

}  // namespace scpf
