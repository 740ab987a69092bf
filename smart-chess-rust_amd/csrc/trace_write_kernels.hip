// trace_write_kernels.hip -- trace files written on the device (sc_traces_format, sc_selfplay_traces_json; the contract is
// include/sc_engine.h's): search records -> the bytes of sctrace::trace_to_json (trace_json.hpp), formatted by trace_fmt.hpp.
//
// ONE wavefront (a workgroup of 64 threads) serves one ply, lane = child, in rounds of 64 children: four rounds at most.
// Two passes over the same formatting code, as the reader has them:
//   k_trace_write<false>   counts: every lane the bytes of its child, the wave's sum with the step's head and tail is the ply's
//                          segment length.  The one scan (scan_kernels.hip) turns the lengths of heads, plies and tails into offsets.
//   k_trace_write<true>    writes: the lane lengths, counted again by the same function, go through an exclusive scan inside
//                          the wave; every lane formats its child into LDS at its place; the wave then moves the round to the
//                          text with 16-byte stores on the 16-byte grid of the output buffer -- the round is staged at the
//                          buffer's alignment, so an aligned LDS read feeds an aligned store.  Only the up to 15 bytes in front
//                          of the first grid line and behind the last one of a round go out as byte stores (a byte store costs
//                          as much fabric time as a 16-byte one: MI355X store rates), about 30 bytes in 4 KB of a usual ply.
//   k_trace_frames         the heads and tails, whose text the host built: one wave per frame, through the same staging.
// These kernels run while the self-play step launches are in flight (held ring rows are final), whose workgroups wait for each
// other inside a launch.  So a writer workgroup waits for nothing outside itself: no spin, no flag, no atomics between
// workgroups; it is one wave, runs for microseconds and takes 9 KB of LDS.
#include <hip/hip_runtime.h>

#include "launchers.hpp"
#include "trace_fmt.hpp"
#include "wave_util.hpp"

namespace sctw {

// `n` staged bytes at stage + (at & 15) -> text[at .. at + n): the whole 16-byte lines with one 16-byte store each, the ragged
// ends bytewise.  Every lane of the wave calls it; the staged bytes must be visible (wave_sync)
__device__ __forceinline__ void flush(char* text, uint32_t at, const char* stage, uint32_t n, int lane) {
    const uint32_t a = at & 15u;
    const uint32_t front = min(n, (16u - a) & 15u);   // bytes in front of the first grid line
    const uint32_t lines = (n - front) >> 4, back = (n - front) & 15u;
    if ((uint32_t)lane < front) text[at + lane] = stage[a + lane];
    const uint4* s16 = reinterpret_cast<const uint4*>(stage + a + front);   // (a + front is 0 or 16)
    uint4* t16 = reinterpret_cast<uint4*>(text + at + front);
    for (uint32_t i = (uint32_t)lane; i < lines; i += 64) t16[i] = s16[i];
    const uint32_t tail = front + (lines << 4);
    if ((uint32_t)lane < back) text[at + tail + lane] = stage[a + tail + lane];
}

template <bool EMIT>
__global__ __launch_bounds__(64) void k_trace_write(Plies P, Steps S, uint32_t* seg_len, Out O) {
    __shared__ __attribute__((aligned(16))) char stage[STAGE_BYTES];
    const uint32_t p = blockIdx.x;
    if (p >= P.n) return;
    const int lane = (int)threadIdx.x;
    const uint32_t src = P.src[p], s = src & ~LAST_PLY;
    const bool last_ply = (src & LAST_PLY) != 0;
    size_t c0;
    int nc;
    if (S.child_off) {
        c0 = S.child_off[s];
        nc = (int)(S.child_off[s + 1] - S.child_off[s]);
    } else {
        c0 = (size_t)s * MAX_CHILDREN;
        nc = S.n_child[s];
    }
    nc = min(max(nc, 0), MAX_CHILDREN);
    const uint16_t move = S.move[s];
    const uint32_t q = S.q[s];
    scfmt::CountSink head, tail;
    scfmt::fmt_step_head(head, move, q, nc > 0);
    scfmt::fmt_step_tail(tail, nc > 0, last_ply);
    const int rounds = max((nc + ROUND - 1) / ROUND, 1);
    uint32_t at = EMIT ? O.seg_off[P.seg[p]] : 0u;   // where the next round goes
    uint32_t total = 0;
    for (int r = 0; r < rounds; r++) {
        const int c = r * ROUND + lane;
        const bool has = c < nc;
        uint16_t cm = 0;
        int32_t cn = 0;
        uint32_t cq = 0, cu = 0;
        if (has) {
            cm = S.child_move[c0 + c];
            cn = S.child_n[c0 + c];
            cq = S.child_q[c0 + c];
            cu = S.child_u[c0 + c];
        }
        scfmt::CountSink mine;
        if (has) scfmt::fmt_child(mine, cm, cn, cq, cu, c + 1 == nc);
        uint32_t sum;
        const uint32_t before = scw::wave_excl_scan_u32(mine.n, &sum);
        const uint32_t front = r == 0 ? head.n : 0u, back = r + 1 == rounds ? tail.n : 0u;
        const uint32_t n_round = front + sum + back;
        if (EMIT) {
            char* base = stage + (at & 15u);
            if (lane == 0 && front) {
                scfmt::BufSink w{base};
                scfmt::fmt_step_head(w, move, q, nc > 0);
            }
            if (has) {
                scfmt::BufSink w{base + front + before};
                scfmt::fmt_child(w, cm, cn, cq, cu, c + 1 == nc);
            }
            if (lane == 0 && back) {
                scfmt::BufSink w{base + front + sum};
                scfmt::fmt_step_tail(w, nc > 0, last_ply);
            }
            scw::wave_sync();
            flush(O.text, at, stage, n_round, lane);
            scw::wave_sync();   // (the next round overwrites the stage)
            at += n_round;
        }
        total += n_round;
    }
    if (!EMIT && lane == 0) seg_len[P.seg[p]] = total;
}

__global__ __launch_bounds__(64) void k_trace_frames(Frames F, Out O) {
    __shared__ __attribute__((aligned(16))) char stage[STAGE_BYTES];
    const uint32_t f = blockIdx.x;
    if (f >= F.n) return;
    const int lane = (int)threadIdx.x;
    const char* text = F.blob + F.off[f];
    const uint32_t len = F.off[f + 1] - F.off[f];
    uint32_t at = O.seg_off[F.seg[f]];
    for (uint32_t done = 0; done < len;) {
        const uint32_t n = min(len - done, (uint32_t)STAGE_BYTES - 16u);
        char* base = stage + (at & 15u);
        for (uint32_t i = (uint32_t)lane; i < n; i += 64) base[i] = text[done + i];
        scw::wave_sync();
        flush(O.text, at, stage, n, lane);
        scw::wave_sync();
        done += n;
        at += n;
    }
}

}  // namespace sctw

namespace scl {
void trace_write_count(const sctw::Plies& p, const sctw::Steps& s, uint32_t* d_seg_len, hipStream_t st) {
    if (p.n == 0) return;
    hipLaunchKernelGGL(sctw::k_trace_write<false>, dim3(p.n), dim3(64), 0, st, p, s, d_seg_len, sctw::Out{nullptr, nullptr});
}
void trace_write_emit(const sctw::Plies& p, const sctw::Steps& s, const sctw::Frames& f, const sctw::Out& o, hipStream_t st) {
    if (f.n) hipLaunchKernelGGL(sctw::k_trace_frames, dim3(f.n), dim3(64), 0, st, f, o);
    if (p.n) hipLaunchKernelGGL(sctw::k_trace_write<true>, dim3(p.n), dim3(64), 0, st, p, s, static_cast<uint32_t*>(nullptr), o);
}
}  // namespace scl
