// trace_fmt.hpp -- the numbers and moves of a trace file as text, ONE source for the host and the device (trace_write_kernels.hip,
// sc_trace_format_f32, tools/trace_fmt_check.cpp).  Integer arithmetic only: no floating-point instruction and no printf, so the
// two sides cannot differ.  The yardstick is trace_json.hpp's fmt_f64 (std::to_chars laid out like ryu::Buffer::format).
//
// fmt_f32 takes a float32 BIT PATTERN and writes the shortest decimal that reads back as the float64 the float widens to:
//   * decode: sign, 8-bit exponent, 23-bit fraction -> m2 * 2^ex with m2 in [2^52, 2^53), the float64's significand (a float32
//     subnormal is a float64 normal: its leading bit is moved up by hand).  m2 is always even, so both ends of the rounding
//     interval belong to it (ryu's acceptBounds).
//   * the interval, in units of 2^(ex - 2): value 4 m2, upper end 4 m2 + 2, lower end 4 m2 - 2 (4 m2 - 1 at a power of two, where
//     the float64 below is half as far away).
//   * ex - 2 >= 0 (at most 73): the three are integers below 2^128, taken as they are.
//     ex - 2 = -s < 0 (s at most 203): x * 2^-s = x * 5^s / 10^s.  As ryu does, q decimal digits are dropped at once --
//     floor(x * 5^(s-q) / 2^q) with q one less than ryu's choice, so that the digit loop below always drops one more digit and
//     sees it -- but the product is EXACT (at most 55 + 149 bits, eight 32-bit words) where ryu multiplies by a truncated
//     128-bit table entry; whether the dropped bits were all zero is read off the product.  No table: 5^(s-q) is built from
//     factors 5^13 < 2^32.
//   * ryu's general digit loop on the three 128-bit integers: drop digits while the ends still differ above them, then the
//     zeros of an exact lower end, round half to even on the last dropped digit.
//   * the digits (at most 17) in ryu's pretty layout, the five cases of fmt_f64.
// The longest text has 24 bytes (-0.000015258788153005298).
#pragma once
#include <stdint.h>

#ifndef SC_HD   // (chess_rules.hpp's)
#if defined(__HIPCC__)
#define SC_HD __host__ __device__ inline
#else
#define SC_HD inline
#endif
#endif

namespace scfmt {

constexpr int F32_MAX_TEXT = 24;    // fmt_f32
constexpr int CHILD_MAX_TEXT = 134; // one child of a trace file: 133 with a count of 10 digits, one more for a minus sign

// ------------------------------------------------------------------ sinks: where text goes
struct CountSink {   // the length only
    uint32_t n = 0;
    SC_HD void put(char) { n++; }
};
struct BufSink {     // into memory
    char* p;
    uint32_t n = 0;
    SC_HD void put(char c) { p[n++] = c; }
};
template <class S>
SC_HD void put_lit(S& s, const char* t) {
    for (; *t; t++) s.put(*t);
}
template <class S>
SC_HD void put_rep(S& s, char c, int n) {
    for (int i = 0; i < n; i++) s.put(c);
}

// ------------------------------------------------------------------ integers
// the decimal digits of v, least significant first, four bits each: 16 in lo, the 17th in hi; returns their number (1 for 0)
struct Bcd {
    uint64_t lo = 0;
    uint32_t hi = 0;
    int len = 0;
    SC_HD int at(int i) const { return i < 16 ? (int)((lo >> (4 * i)) & 15) : (int)hi; }   // digit i, 0 = least significant
};
SC_HD Bcd to_bcd(uint64_t v) {
    Bcd b;
    do {
        const uint64_t q = v / 10;
        const uint32_t d = (uint32_t)(v - q * 10);
        if (b.len < 16) b.lo |= (uint64_t)d << (4 * b.len);
        else b.hi = d;
        b.len++;
        v = q;
    } while (v);
    return b;
}
template <class S>
SC_HD void fmt_u32(S& s, uint32_t v) {
    const Bcd b = to_bcd(v);
    for (int i = b.len - 1; i >= 0; i--) s.put((char)('0' + b.at(i)));
}
template <class S>
SC_HD void fmt_i32(S& s, int32_t v) {   // std::to_string(int)
    if (v < 0) s.put('-');
    fmt_u32(s, v < 0 ? 0u - (uint32_t)v : (uint32_t)v);
}
// UCI text of a move (sctrace::move_uci)
template <class S>
SC_HD void fmt_move(S& s, uint16_t m) {
    const int f = m & 63, t = (m >> 6) & 63, pr = (m >> 12) & 7;
    s.put((char)('a' + (f & 7)));
    s.put((char)('1' + (f >> 3)));
    s.put((char)('a' + (t & 7)));
    s.put((char)('1' + (t >> 3)));
    if (pr >= 2 && pr <= 5) s.put(pr == 2 ? 'n' : pr == 3 ? 'b' : pr == 4 ? 'r' : 'q');
}

// ------------------------------------------------------------------ multi-word integers, little-endian 32-bit words
template <int W>
struct Big {
    uint32_t w[W];
};
template <int W>
SC_HD void big_mul_small(Big<W>& a, uint32_t f) {
    uint64_t carry = 0;
    for (int i = 0; i < W; i++) {
        const uint64_t t = (uint64_t)a.w[i] * f + carry;
        a.w[i] = (uint32_t)t;
        carry = t >> 32;
    }
}
// a /= 10, returns a % 10
SC_HD uint32_t big_div10(Big<4>& a) {
    uint32_t r = 0;
    for (int i = 3; i >= 0; i--) {
        const uint64_t cur = ((uint64_t)r << 32) | a.w[i];
        const uint64_t q = cur / 10;
        a.w[i] = (uint32_t)q;
        r = (uint32_t)(cur - q * 10);
    }
    return r;
}
SC_HD int big_cmp(const Big<4>& a, const Big<4>& b) {
    for (int i = 3; i >= 0; i--)
        if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
    return 0;
}
// x (below 2^56) << sh, sh < 74
SC_HD Big<4> big_from_shl(uint64_t x, int sh) {
    Big<4> r;
    const uint32_t src[2] = {(uint32_t)x, (uint32_t)(x >> 32)};
    const int ws = sh >> 5, bs = sh & 31;
    for (int i = 0; i < 4; i++) {
        const int k = i - ws;
        uint64_t v = 0;
        if (k >= 0 && k < 2) v |= (uint64_t)src[k] << bs;
        if (k - 1 >= 0 && k - 1 < 2) v |= ((uint64_t)src[k - 1] << bs) >> 32;
        r.w[i] = (uint32_t)v;
    }
    return r;
}
// floor(a / 2^q) (which fits four words); *exact: no bit was dropped.  q < 160
SC_HD Big<4> big_shr(const Big<8>& a, int q, bool* exact) {
    const int ws = q >> 5, bs = q & 31;
    uint32_t dropped = bs ? (a.w[ws] & ((1u << bs) - 1u)) : 0u;
    for (int i = 0; i < ws; i++) dropped |= a.w[i];
    *exact = dropped == 0;
    Big<4> r;
    for (int i = 0; i < 4; i++) {
        const int k = i + ws;
        const uint64_t lo = k < 8 ? a.w[k] : 0u, hi = k + 1 < 8 ? a.w[k + 1] : 0u;
        r.w[i] = (uint32_t)(((hi << 32) | lo) >> bs);
    }
    return r;
}

// ------------------------------------------------------------------ float32 bit pattern -> text
// the shortest digits of the float64 that `bits` widens to (a finite value that is not zero): value = digits * 10^exp10, the
// digits without trailing zeros
SC_HD uint64_t shortest_digits(uint32_t bits, int* exp10) {
    const uint32_t e8 = (bits >> 23) & 255u, frac = bits & 0x7FFFFFu;
    uint64_t m2;
    int ex;   // value = m2 * 2^ex, m2 in [2^52, 2^53)
    if (e8) {
        m2 = ((uint64_t)1 << 52) | ((uint64_t)frac << 29);
        ex = (int)e8 - 127 - 52;
    } else {   // frac * 2^-149, frac != 0: its leading bit goes to bit 52
        int top = 22;
        while (!((frac >> top) & 1u)) top--;
        m2 = (uint64_t)frac << (52 - top);
        ex = -149 - (52 - top);
    }
    const int e2 = ex - 2;
    const uint64_t mv = 4 * m2;
    const uint32_t below = m2 != ((uint64_t)1 << 52) ? 2u : 1u;   // (a widened float32 is never the smallest float64 binade)
    Big<4> vr, vp, vm;
    bool vm_exact = true, vr_exact = true;
    int e10 = 0;
    if (e2 >= 0) {
        vr = big_from_shl(mv, e2);
        vp = big_from_shl(mv + 2, e2);
        vm = big_from_shl(mv - below, e2);
    } else {
        const int s = -e2;
        const int q_ryu = (int)(((uint32_t)s * 732923u) >> 20) - (s > 1);   // floor(s * log10(5)) - (s > 1)
        const int q = q_ryu > 0 ? q_ryu - 1 : 0;
        int i = s - q;   // at most 64
        Big<8> a{{(uint32_t)mv, (uint32_t)(mv >> 32), 0, 0, 0, 0, 0, 0}}, b{{1u, 0, 0, 0, 0, 0, 0, 0}};   // mv * 5^i, 5^i
        for (; i >= 13; i -= 13) {
            big_mul_small(a, 1220703125u);   // 5^13
            big_mul_small(b, 1220703125u);
        }
        uint32_t f = 1;
        for (; i > 0; i--) f *= 5u;
        big_mul_small(a, f);
        big_mul_small(b, f);
        Big<8> hi = a, lo = a;   // a + 2 b, a - below * b
        uint64_t carry = 0;
        int64_t borrow = 0;
        for (int k = 0; k < 8; k++) {
            const uint64_t t = (uint64_t)hi.w[k] + 2ull * b.w[k] + carry;
            hi.w[k] = (uint32_t)t;
            carry = t >> 32;
            const int64_t d = (int64_t)lo.w[k] - (int64_t)((uint64_t)below * b.w[k]) + borrow;
            lo.w[k] = (uint32_t)d;
            borrow = d >> 32;   // (arithmetic shift: 0 or negative)
        }
        bool vp_exact;
        vr = big_shr(a, q, &vr_exact);
        vp = big_shr(hi, q, &vp_exact);
        vm = big_shr(lo, q, &vm_exact);
        e10 = q - s;
    }
    // ryu's general loop (d2s.c, acceptBounds = true)
    uint32_t last = 0;
    for (;;) {
        Big<4> p10 = vp, m10 = vm;
        big_div10(p10);
        const uint32_t vm_mod = big_div10(m10);
        if (big_cmp(p10, m10) <= 0) break;
        vm_exact = vm_exact && vm_mod == 0;
        vr_exact = vr_exact && last == 0;
        last = big_div10(vr);
        vp = p10;
        vm = m10;
        e10++;
    }
    if (vm_exact) {
        for (;;) {
            Big<4> m10 = vm;
            if (big_div10(m10) != 0) break;
            vr_exact = vr_exact && last == 0;
            last = big_div10(vr);
            big_div10(vp);
            vm = m10;
            e10++;
        }
    }
    if (vr_exact && last == 5 && (vr.w[0] & 1u) == 0) last = 4;   // round half to even
    uint64_t out = ((uint64_t)vr.w[1] << 32) | vr.w[0];          // (17 digits at most)
    if ((big_cmp(vr, vm) == 0 && !vm_exact) || last >= 5) out++;
    for (;;) {   // 9.5 rounded up to 10
        const uint64_t t = out / 10;
        if (t * 10 != out) break;
        out = t;
        e10++;
    }
    *exp10 = e10;
    return out;
}

// fmt_f64((double)f) of the float with these bits
template <class S>
SC_HD void fmt_f32(S& s, uint32_t bits) {
    if (((bits >> 23) & 255u) == 255u) {
        put_lit(s, "null");
        return;
    }
    if (bits >> 31) s.put('-');
    if ((bits & 0x7FFFFFFFu) == 0) {
        put_lit(s, "0.0");
        return;
    }
    int k;   // value = digits * 10^k
    const Bcd d = to_bcd(shortest_digits(bits, &k));
    const int len = d.len, kk = k + len;   // value = 0.DIGITS * 10^kk
    if (0 <= k && kk <= 16) {
        for (int i = len - 1; i >= 0; i--) s.put((char)('0' + d.at(i)));
        put_rep(s, '0', k);
        put_lit(s, ".0");
    } else if (0 < kk && kk <= 16) {
        for (int i = len - 1; i >= 0; i--) {
            if (i == len - 1 - kk) s.put('.');
            s.put((char)('0' + d.at(i)));
        }
    } else if (-5 < kk && kk <= 0) {
        put_lit(s, "0.");
        put_rep(s, '0', -kk);
        for (int i = len - 1; i >= 0; i--) s.put((char)('0' + d.at(i)));
    } else {
        s.put((char)('0' + d.at(len - 1)));
        if (len > 1) {
            s.put('.');
            for (int i = len - 2; i >= 0; i--) s.put((char)('0' + d.at(i)));
        }
        s.put('e');
        fmt_i32(s, kk - 1);
    }
}

// ------------------------------------------------------------------ the pieces of a trace file that kernels write
// one child of a step: [uci, N, Q_sum, uct] in serde_json's pretty form at depth 4, with what separates it from the next
template <class S>
SC_HD void fmt_child(S& s, uint16_t move, int32_t n, uint32_t q_bits, uint32_t u_bits, bool last) {
    put_lit(s, "        [\n          \"");
    fmt_move(s, move);
    put_lit(s, "\",\n          ");
    fmt_i32(s, n);
    put_lit(s, ",\n          ");
    fmt_f32(s, q_bits);
    put_lit(s, ",\n          ");
    fmt_f32(s, u_bits);
    put_lit(s, last ? "\n        ]\n" : "\n        ],\n");
}
// a step in front of its children and behind them
template <class S>
SC_HD void fmt_step_head(S& s, uint16_t move, uint32_t q_bits, bool has_children) {
    put_lit(s, "    [\n      \"");
    fmt_move(s, move);
    put_lit(s, "\",\n      ");
    fmt_f32(s, q_bits);
    put_lit(s, has_children ? ",\n      [\n" : ",\n      []");
}
template <class S>
SC_HD void fmt_step_tail(S& s, bool has_children, bool last) {
    if (has_children) put_lit(s, "      ]");
    put_lit(s, last ? "\n    ]\n" : "\n    ],\n");
}

}  // namespace scfmt
