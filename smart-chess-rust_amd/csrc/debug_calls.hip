// debug_calls.hip -- host side of libsc_engine.so: test and developer aids (sc_debug_find_max, sc_debug_choose_child,
// sc_selfplay_debug_cycles).  The two aids that touch the single-launch stream grant are beside it, in selfplay.hip.
#include <string.h>

#include <map>

#include "host_common.hpp"

extern "C" {

int sc_debug_find_max(int device_id, const float* values, int n, int32_t* out2) {
    if (!values || !out2 || n < 1 || n > 256) return fail("bad argument");
    TRY(use_device(nullptr, device_id));
    ScopedDev<float> d_u;
    ScopedDev<int> d_o;
    HIPOK(d_u.alloc(256));
    HIPOK(d_o.alloc(2));
    HIPOK(hipMemcpy(d_u.p, values, (size_t)n * 4, hipMemcpyHostToDevice));
    scl::debug_find_max(d_u.p, n, d_o.p, nullptr);
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpy(out2, d_o.p, 8, hipMemcpyDeviceToHost));
    return 0;
}

int sc_debug_choose_child(int device_id, int n_cases, const int32_t* n_act, const int32_t* nc, const float* temperature, const float* u,
                          int tie_random, int32_t* choice_out, float* total_out) {
    if (!n_act || !nc || !temperature || !u || !choice_out || !total_out || n_cases < 1 || n_cases > (1 << 20)) return fail("bad argument");
    int w_max = 0;
    for (int c = 0; c < n_cases; c++) {
        if (nc[c] < 1 || nc[c] > sc::MAXC) return fail("sc_debug_choose_child: nc out of [1, 224]");
        if (!(temperature[c] >= 0.0f) || !(u[c] >= 0.0f && u[c] < 1.0f)) return fail("sc_debug_choose_child: temperature < 0 or u outside [0, 1)");
        for (int i = 0; i < nc[c]; i++) {
            const int32_t n = n_act[(size_t)c * sc::MAXC + i];
            if (n < 0 || n > 60000) return fail("sc_debug_choose_child: visit count out of [0, 60000]");
            w_max = std::max(w_max, (int)n);
        }
    }
    // one weight table per distinct temperature, made by the function that makes a self-play handle's
    std::vector<float> w(1, 0.0f);
    std::vector<int32_t> w_off((size_t)n_cases, 0);
    std::map<uint32_t, int32_t> table_of;
    for (int c = 0; c < n_cases; c++) {
        if (temperature[c] == 0.0f) continue;
        uint32_t bits;
        memcpy(&bits, &temperature[c], 4);
        auto it = table_of.find(bits);
        if (it == table_of.end()) {
            if (table_of.size() >= 64) return fail("sc_debug_choose_child: more than 64 distinct temperatures");
            it = table_of.emplace(bits, (int32_t)w.size()).first;
            const std::vector<float> t = choice_weights(temperature[c], w_max);
            w.insert(w.end(), t.begin(), t.end());
        }
        w_off[(size_t)c] = it->second;
    }
    TRY(use_device(nullptr, device_id));
    const size_t n = (size_t)n_cases;
    ScopedDev<int32_t> d_n, d_nc, d_ch, d_off;
    ScopedDev<float> d_t, d_u, d_tot, d_w;
    HIPOK(d_n.alloc(n * sc::MAXC));
    HIPOK(d_nc.alloc(n));
    HIPOK(d_ch.alloc(n));
    HIPOK(d_off.alloc(n));
    HIPOK(d_t.alloc(n));
    HIPOK(d_u.alloc(n));
    HIPOK(d_tot.alloc(n));
    HIPOK(d_w.alloc(w.size()));
    HIPOK(hipMemcpy(d_n.p, n_act, n * sc::MAXC * 4, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_nc.p, nc, n * 4, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_t.p, temperature, n * 4, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_u.p, u, n * 4, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_off.p, w_off.data(), n * 4, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_w.p, w.data(), w.size() * 4, hipMemcpyHostToDevice));
    scl::debug_choose_child(n_cases, d_n.p, d_nc.p, d_t.p, d_u.p, tie_random ? 1 : 0, d_w.p, d_off.p, w_max, d_ch.p, d_tot.p, nullptr);
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpy(choice_out, d_ch.p, n * 4, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(total_out, d_tot.p, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

/* developer aid: cycle stamps of the last k_mcts launch, out[n_slots][8] */
int sc_selfplay_debug_cycles(sc_selfplay* sp, int enable, unsigned long long* out) {
    if (!sp) return fail("null handle");
    HIPOK(hipSetDevice(sp->device));
    if (enable && !sp->p.dbg_cycles) TRY(sp_alloc(sp, &sp->p.dbg_cycles, (size_t)sp->p.n_slots * 32));
    HIPOK(hipStreamSynchronize(sp->stream));
    if (out && sp->p.dbg_cycles)
        HIPOK(hipMemcpy(out, sp->p.dbg_cycles, (size_t)sp->p.n_slots * 256, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
