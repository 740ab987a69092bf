// trace_types.hpp -- kernel argument blocks of the trace-file reader (trace_kernels.hip), shared by host code and kernels.  Every
// pointer is device memory.
#pragma once
#include <stdint.h>

namespace sctr {

constexpr int CHUNK = 4096;          // bytes of a file one workgroup of 256 threads reads at a time, 16 per thread
constexpr int FEN_CAP = 128;         // a file's "fen" member: at most 127 bytes and the final zero
constexpr uint32_t MAX_PLIES = 4000, MAX_CHILDREN = 224, MAX_SPACE = 255;

// the text of n files: file g is text[off[g] .. off[g + 1]).  text is 16-byte aligned and 16 bytes behind off[n] can be read: the
// chunks are cut on the 16-byte grid of the buffer, not of the file
struct Text {
    int n;
    const char* text;
    const uint64_t* off;   // [n + 1]
};
// per file, written by the counting pass.  status 0 or -code, the counts 0 for a refused file
struct Files {
    int32_t* status;
    uint32_t* err_at;
    uint32_t *n_steps, *n_children, *n_opening;
    int32_t* outcome;   // [n][3]: has_outcome, termination, winner
    int32_t* has_fen;
    char* fen;          // [n][FEN_CAP]
};
// the packed arrays of the set and the files' bases in them (the exclusive scans of the counts)
struct Packed {
    const uint32_t *step_base, *child_base, *open_base;
    uint16_t* moves;
    uint32_t* child_off;   // [plies]: global, into child_mv / child_n
    uint16_t* child_mv;
    uint32_t* child_n;
    uint16_t* opening;
};

}  // namespace sctr
