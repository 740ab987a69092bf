// trace_fmt_check.cpp -- stand-alone check of the trace writer's number formatter (csrc/trace_fmt.hpp) against the host writer's
// fmt_f64 (csrc/trace_json.hpp: std::to_chars laid out like ryu), host only:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Ismart-chess-rust_amd/csrc
//       tools/trace_fmt_check.cpp -o trace_fmt_check && ./trace_fmt_check
//   g++ -std=c++17 -O2 -pthread -Ismart-chess-rust_amd/csrc tools/trace_fmt_check.cpp -o trace_fmt_check && ./trace_fmt_check --all
//
// Without an argument: the edge set (every exponent x a few fractions x both signs, the layout boundaries) and a strided sweep
// of the 2^32 bit patterns, each text written into a heap block of exactly 24 bytes -- a 25th byte is outside the block, which
// the sanitizer reports.  --all: every one of the 2^32 patterns, on 16 threads (no sanitizer: minutes, not hours).
// Also the counts and moves against std::to_string and sctrace::move_uci.  Exit code 0: no mismatch.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "trace_fmt.hpp"
#include "trace_json.hpp"

static std::atomic<unsigned long long> g_bad{0};
static std::atomic<int> g_longest{0};

static void check(uint32_t bits) {
    float f;
    memcpy(&f, &bits, 4);
    const std::string want = sctrace::fmt_f64((double)f);
    std::unique_ptr<char[]> block(new char[scfmt::F32_MAX_TEXT]);
    scfmt::CountSink c;
    scfmt::fmt_f32(c, bits);
    bool ok = c.n <= (uint32_t)scfmt::F32_MAX_TEXT && c.n == want.size();
    if (ok) {
        scfmt::BufSink b{block.get()};
        scfmt::fmt_f32(b, bits);
        ok = b.n == c.n && memcmp(block.get(), want.data(), want.size()) == 0;
    }
    int len = (int)c.n, cur = g_longest.load();
    while (len > cur && !g_longest.compare_exchange_weak(cur, len)) {}
    if (!ok && g_bad.fetch_add(1) < 20) fprintf(stderr, "0x%08x: want %s, counted %u bytes\n", bits, want.c_str(), c.n);
}

static void edge_set() {
    static const uint32_t FRAC[] = {0u, 1u, 0x400000u, 0x7FFFFFu, 0x2AAAAAu, 0x555555u, 0x000100u};
    for (uint32_t e = 0; e < 256; e++)
        for (uint32_t f : FRAC)
            for (uint32_t s = 0; s < 2; s++) check((s << 31) | (e << 23) | f);
    // the layout boundaries 1e-5, 1e16, 1e17 and the patterns around them; the subnormals' leading bits
    for (float v : {1e-5f, 9.9999e-6f, 1e-4f, 1e16f, 1e17f, 9.9999998e15f, 1e15f, 0.5f, 1.0f, 16777216.0f, 3.4028235e38f, 1.1754944e-38f}) {
        uint32_t b;
        memcpy(&b, &v, 4);
        for (int d = -64; d <= 64; d++) check(b + (uint32_t)d), check((b + (uint32_t)d) | 0x80000000u);
    }
    for (int top = 0; top < 23; top++)
        for (uint32_t low : {0u, 1u, 0x155555u}) check((1u << top) | (low & ((1u << top) - 1u)));
}

static void ints_and_moves() {
    for (uint64_t v : {0ull, 9ull, 10ull, 99ull, 100ull, 999ull, 1000ull, 65535ull, 999999999ull, 1000000000ull, 2147483647ull, 4294967295ull}) {
        char buf[16];
        scfmt::BufSink b{buf};
        scfmt::fmt_u32(b, (uint32_t)v);
        if (std::string(buf, b.n) != std::to_string(v)) g_bad++;
    }
    for (int32_t v : {0, -1, 7, -2147483647 - 1, 2147483647}) {
        char buf[16];
        scfmt::BufSink b{buf};
        scfmt::fmt_i32(b, v);
        if (std::string(buf, b.n) != std::to_string(v)) g_bad++;
    }
    for (uint32_t m = 0; m < 65536; m++) {
        char want[8], buf[8];
        const int n = sctrace::move_uci((uint16_t)m, want);
        scfmt::BufSink b{buf};
        scfmt::fmt_move(b, (uint16_t)m);
        if ((int)b.n != n || memcmp(buf, want, (size_t)n) != 0) g_bad++;
    }
}

int main(int argc, char** argv) {
    const bool all = argc > 1 && strcmp(argv[1], "--all") == 0;
    edge_set();
    ints_and_moves();
    unsigned long long n = 0;
    if (all) {
        std::vector<std::thread> th;
        for (uint32_t t = 0; t < 16; t++)
            th.emplace_back([t] {
                for (uint64_t b = (uint64_t)t << 28; b < ((uint64_t)t + 1) << 28; b++) check((uint32_t)b);
            });
        for (auto& x : th) x.join();
        n = 1ull << 32;
    } else {
        for (uint64_t b = 0; b < (1ull << 32); b += 20011) check((uint32_t)b), n++;   // a prime stride: every exponent, mixed fractions
    }
    printf("%llu patterns of the sweep, %llu mismatches, longest text %d bytes\n", n, g_bad.load(), g_longest.load());
    return g_bad.load() ? 1 : 0;
}
