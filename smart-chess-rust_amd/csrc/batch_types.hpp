// batch_types.hpp -- kernel argument block of the minibatch gather (batch_kernels.hip), shared by host code and kernel.
#pragma once
#include <stdint.h>

namespace scbt {

constexpr int PLANES = 112;      // int8 planes per square
constexpr int CELLS = 7168;      // 64 squares x 112 planes
constexpr int ROW = 4672;        // actions per position
constexpr int ROW4 = ROW / 4;    // ... as 16-byte stores: 1168 = 4 * 256 + 144
constexpr int LEGAL_ROW = 224;   // SC_MAX_MOVES
constexpr int MAX_LEGAL = 218;

// sc_gather_batch: sample b of the batch is built from row rows[b] of the compact tensors (layout 0 of sc_encode_steps_device)
struct GatherArgs {
    int n_src;
    int n_batch;
    const int32_t* rows;         // [n_batch]
    const uint8_t* mirror;       // [n_batch] or null
    const int8_t* boards;        // [n_src][8][8][112]
    const int32_t* meta;         // [n_src][7]
    const float* dist_legal;     // [n_src][224]
    const uint16_t* legal_idx;   // [n_src][224]
    const int32_t* n_legal;      // [n_src]
    const float* outcome;        // [n_src]
    float* out_boards;           // [n_batch][112][8][8], or null (as every output)
    float* out_meta;             // [n_batch][7]
    float* out_dist;             // [n_batch][4672]
    float* out_outcome;          // [n_batch]
    int32_t* n_bad;              // [1]
};

}  // namespace scbt
