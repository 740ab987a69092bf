// advance_types.hpp -- the argument block of k_advance (advance_kernels.hip), filled by sc_selfplay_advance (advance.hip).
#pragma once
#include <stdint.h>

namespace scad {

constexpr int ADV_THREADS = 256;        // one workgroup per listed slot; its chunk of the sweep: one node per thread
constexpr int PS_WORDS = 65536 / 32;    // the kept tpos slots as a bitmap in LDS (NodeHdr::ps is 16 bits wide): 8 KB

// Entry i plays moves[i] in slot slots[i].  scratch: one word per LIVE node of the listed slots -- entry i owns
// scratch[off[i] .. off[i + 1]), off[i + 1] - off[i] being the slot's n_nodes as the host read it -- zeroed by the host; the kernel
// leaves 0 for a node outside the kept subtree and 1 + its new index for a kept one.  kept: int32 [n][3] (n_nodes, n_exp, the new
// root's visits; zeros where the status is not 0)
struct AdvanceArgs {
    int n;
    const int32_t* slots;
    const uint16_t* moves;
    int32_t* status;
    int32_t* kept;
    uint32_t* scratch;
    const uint64_t* off;   // [n + 1]
};

}  // namespace scad
