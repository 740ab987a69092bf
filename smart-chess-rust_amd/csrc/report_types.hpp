// report_types.hpp -- the search report read from the trees on the device (report_kernels.hip, report.hip), shared by host code and
// kernels: the per-slot record, the argument block of the kernel and the layout of the packed buffer it writes.
#pragma once
#include "mcts_types.hpp"

namespace scrp {

constexpr int MAX_PV = 1024;   // a walk never takes more moves: the search's own depth limit (its paths hold 1024 nodes)
enum { END_OPEN = 0, END_DRAW = 1, END_WHITE = 2, END_BLACK = 3, END_DEPTH = 4 };   // the last node of a line (sc_engine.h)

// sc_report_slot of include/sc_engine.h, field for field (report.hip pins the size)
struct SlotInfo {
    int32_t status, ply, sim, n_nodes, n_root_children, root_children_n, root_n, turn, n_lines, pad;
    float root_w;
};

// One report.  The tree pointers are the handle's (copied from its SpParams: the kernel reads the pools in place and writes
// nothing they hold); the outputs are the regions of the handle's packed buffer (Packed below), rows of `multipv` lines per entry.
struct ReportArgs {
    int n, multipv, pv_cap;
    int n_slots, node_cap, hist_cap;
    const int32_t* slots;   // [n] or null: entry i is slot i
    const sc::GameCtl* ctl;
    const sc::Position* hist;
    const int32_t* N;
    const float* W;
    const float* P;
    const uint16_t* MV;
    const sc::NodeHdr* H;
    SlotInfo* info;        // [n]
    int32_t* line_child;   // [n][multipv]
    int32_t* line_n;
    float* line_w;
    float* line_prior;
    int32_t* line_len;
    int32_t* line_end;
    uint16_t* pv;          // [n][multipv][pv_cap]
};

// The packed buffer: the slot list, the slot records, six line arrays and the moves, each region from a 16-byte boundary on, so
// that one copy brings a report to the host
struct Packed {
    size_t slots, info, line[6], pv, bytes;
    Packed(size_t n, size_t multipv, size_t pv_cap) {
        size_t at = 0;
        auto take = [&at](size_t b) {
            const size_t o = at;
            at += (b + 15) & ~(size_t)15;
            return o;
        };
        slots = take(n * 4);
        info = take(n * sizeof(SlotInfo));
        for (size_t& l : line) l = take(n * multipv * 4);
        pv = take(n * multipv * pv_cap * 2);
        bytes = at ? at : 16;
    }
};

}  // namespace scrp
