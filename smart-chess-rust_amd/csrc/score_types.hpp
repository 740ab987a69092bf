// score_types.hpp -- kernel argument blocks of the scoring kernels (score_kernels.hip), shared by host code and kernels.
#pragma once
#include <stdint.h>

namespace scsc {

constexpr int ROW = 4672;        // log-probabilities per position
constexpr int ROW4 = ROW / 4;    // ... as 16-byte loads: 1168 = 18 * 64 + 16
constexpr int LEGAL_ROW = 224;   // SC_MAX_MOVES
constexpr int MAX_LEGAL = 218;

// sc_score_positions, one slice: position p of the slice reads row p of every input and writes entry p of every output
struct ScoreArgs {
    int n;
    const float* logp;          // [n][4672] the tower's log-softmax rows (engine scratch)
    const float* value;         // [n] value_finish's output (engine scratch)
    const float* dist;          // dense form [n][4672], or null
    const float* dist_legal;    // sparse form [n][224] + legal_idx [n][224] + n_legal [n], or null
    const uint16_t* legal_idx;
    const int32_t* n_legal;
    const float* outcome;       // [n]
    float* ce;                  // [n] each: never null here (the host substitutes scratch for outputs the caller does not want)
    float* se;
    float* ent;
    float* value_out;           // [n] or null
};

// sc_compare_engines, one slice
struct CompareArgs {
    int n;
    const float* logp1;
    const float* logp2;
    const float* value1;
    const float* value2;
    float* tv;   // never null
    float* dv;
};

// the [P] -> summary reduction: one workgroup, double precision, fixed order
struct SummaryArgs {
    int n;
    int mode;           // 0: sc_score_positions (x0 = ce, x1 = se, x2 = ent), 1: sc_compare_engines (x0 = tv, x1 = dv)
    const float* x0;
    const float* x1;
    const float* x2;
    double* out;        // mode 0: 5 doubles, mode 1: 9 doubles (include/sc_engine.h)
};

}  // namespace scsc
