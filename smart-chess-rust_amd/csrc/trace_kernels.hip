// trace_kernels.hip -- trace files read on the device (sc_traces_read; the contract is include/sc_engine.h's): the text of n
// files -> played moves, children with visit counts, outcome, "opening" and "fen".  A reader of machine-written traces, not a
// JSON validator.
//
// ONE workgroup of 256 threads serves one file and walks it in chunks of 4 KiB, 16 bytes per thread with one 16-byte load (the
// chunks are cut on the 16-byte grid of the text buffer, bytes outside the file read as spaces); the chunk and the 512 bytes
// behind it also go to LDS.  Four block scans per chunk, each carried from chunk to chunk the way k_scan_sums carries its sum,
// class every byte without looking at its neighbours:
//   quotes (sum)        -> the quote parity of every byte: inside a string or not (strings hold no backslash)
//   brackets (sum)      -> the depth of every byte outside strings
//   keys (max)          -> the depth-1 key in force: (position, key id) of the last string in the top object that follows '{' or ','
//   events (Cnt)        -> the running numbers of steps, children and opening moves, and the children since the last step:
//                          '[' at depth 3 / 5 under "steps" opens a step / a child, a string at depth 2 under "opening" is a move
// The thread that owns an event then does what cannot be done bytewise, with a bounded sequential read (from the LDS window; the
// few reads that leave it go to memory): checks and packs the move, steps over white space and the comma, parses the count,
// checks the shape.  The first defect of a file is folded by a 64-bit atomic min on (offset << 8 | code) in LDS.
// Two passes over the text, the same walk: k_trace<false> counts and checks (per file: status, counts, outcome, fen),
// k_trace<true> writes the packed arrays at base + running index, the bases being the exclusive scans of the counts.
// A single very large file runs on one workgroup (13 MB worst case: ~3 300 chunks per pass); the workload is thousands of files
// of 0.1 - 0.5 MB.
#include <hip/hip_runtime.h>

#include "../../include/sc_engine.h"
#include "launchers.hpp"

namespace sctr {

enum Key { K_OTHER = 0, K_STEPS = 1, K_OUTCOME = 2, K_OPENING = 3, K_FEN = 4 };
// what a byte starts.  NEED_*: the next token after this bracket or comma must be one of the two characters
enum Ev { EV_NONE = 0, EV_STEP, EV_CHILD, EV_OPEN_MOVE, EV_KEY_STEPS, EV_KEY_OUTCOME, EV_FEN,
          EV_NEED_ARR_OR_CLOSE,   // '[' of "steps" or of a children array
          EV_NEED_ARR,            // ',' between steps or between children
          EV_NEED_CLOSE,          // ']' of a children array: the step ends behind it
          EV_NEED_STR_OR_CLOSE,   // '[' of "opening"
          EV_NEED_STR };          // ',' between opening moves

__device__ const char TERM_NAMES[11][24] = {"", "Checkmate", "Stalemate", "InsufficientMaterial", "SeventyfiveMoves", "FivefoldRepetition",
                                            "FiftyMoves", "ThreefoldRepetition", "VariantWin", "VariantLoss", "VariantDraw"};

// one file's bytes, and the window of them the workgroup holds in LDS: the chunk it is at and the AHEAD bytes behind it, where
// nearly every sequential read of an event's owner ends; a read outside the window goes to memory
constexpr uint32_t AHEAD = 512, WINDOW = CHUNK + AHEAD;
struct File {
    const unsigned char* p;
    uint32_t len;
    const unsigned char* win;   // LDS
    uint32_t win0;              // the offset in the file of win[0], modulo 2^32 (the first window starts in front of the file)
    __device__ __forceinline__ int at(uint32_t i) const {   // (-1: behind the text)
        if (i >= len) return -1;
        const uint32_t k = i - win0;
        return k < WINDOW ? (int)win[k] : (int)p[i];
    }
};
__device__ __forceinline__ bool is_ws(int c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }
__device__ __forceinline__ bool is_digit(int c) { return c >= '0' && c <= '9'; }

// the sequential reader of an event's owner: the first failure sticks and stops every later step.  A failure at or behind the end
// of the text is the text's: it ends inside a token (UNBALANCED at the file's length)
struct Cur {
    const File& f;
    uint32_t i;
    int code = 0;
    uint32_t where = 0;
    bool eof = false;   // a read went behind the text
    __device__ void fail(int c, uint32_t at) {
        if (code) return;
        const bool ended = eof || i >= f.len;
        code = ended ? SC_TRACE_ERR_UNBALANCED : c;
        where = ended ? f.len : at;
    }
    __device__ int peek() const { return code ? -1 : f.at(i); }
    __device__ void ws() {
        if (code) return;
        uint32_t k = 0;
        while (k <= MAX_SPACE && is_ws(f.at(i + k))) k++;
        if (k > MAX_SPACE) fail(SC_TRACE_ERR_SPACE, i);
        else i += k;
    }
    __device__ bool eat(int c) {
        if (code || f.at(i) != c) return false;
        i++;
        return true;
    }
    __device__ bool lit(const char* s, int n) {
        if (code) return false;
        for (int k = 0; k < n; k++) {
            const int c = f.at(i + (uint32_t)k);
            if (c != s[k]) {
                eof |= c < 0;
                return false;
            }
        }
        i += (uint32_t)n;
        return true;
    }
    // "e2e4" / "a7a8q" with its quotes, at the opening quote
    __device__ uint16_t move() {
        if (code) return 0;
        const uint32_t q = i;
        int c[7];
        int n = 0;   // the bytes of the string, at most 6 of them, up to its closing quote
        for (; n < 6; n++) {
            c[n] = f.at(q + 1 + (uint32_t)n);
            if (c[n] == '"' || c[n] < 0) break;
        }
        eof |= n < 6 && c[n] < 0;
        const int promo = n == 5 ? (c[4] == 'n' ? 2 : c[4] == 'b' ? 3 : c[4] == 'r' ? 4 : c[4] == 'q' ? 5 : -1) : 0;
        const bool ok = f.at(q) == '"' && (n == 4 || n == 5) && c[n] == '"' && (unsigned)(c[0] - 'a') < 8u && (unsigned)(c[1] - '1') < 8u &&
                        (unsigned)(c[2] - 'a') < 8u && (unsigned)(c[3] - '1') < 8u && promo >= 0;
        if (!ok) {
            fail(SC_TRACE_ERR_MOVE, q);
            return 0;
        }
        i = q + 2 + (uint32_t)n;
        return (uint16_t)(((c[1] - '1') * 8 + (c[0] - 'a')) | (((c[3] - '1') * 8 + (c[2] - 'a')) << 6) | (promo << 12));
    }
};

// a step behind its move and comma: [move, number or null, [children]] up to the '[' of the children
__device__ void step_tail(Cur& c) {
    if (!c.lit("null", 4)) {
        int k = 0;
        for (int ch = c.peek(); k < 48 && (is_digit(ch) || ch == '-' || ch == '+' || ch == '.' || ch == 'e' || ch == 'E'); ch = c.peek()) c.i++, k++;
        if (k == 0) c.fail(SC_TRACE_ERR_SHAPE, c.i);
    }
    c.ws();
    if (!c.eat(',')) c.fail(SC_TRACE_ERR_SHAPE, c.i);
    c.ws();
    if (c.peek() != '[') c.fail(SC_TRACE_ERR_SHAPE, c.i);
}
// a child behind its move and comma: [move, count, ...]; what follows the count is not read
__device__ uint32_t child_count(Cur& c) {
    const uint32_t tok = c.i;
    unsigned long long v = 0;
    int nd = 0;
    for (int ch = c.peek(); is_digit(ch) && nd < 11; ch = c.peek()) v = v * 10 + (unsigned)(ch - '0'), nd++, c.i++;
    const int behind = c.peek();
    if (nd == 0 || v > 0xFFFFFFFFull || !(is_ws(behind) || behind == ',' || behind == ']')) c.fail(SC_TRACE_ERR_COUNT, tok);
    return (uint32_t)v;
}
// "outcome", from the key's quote: null, or {"termination": name, "winner": "White" | "Black" | null} in either order
__device__ void parse_outcome(Cur& c, int out[3]) {
    const uint32_t key = c.i;
    int has = 0, term = 0, winner = -2;
    c.i += 9;
    c.ws();
    if (!c.eat(':')) c.fail(SC_TRACE_ERR_OUTCOME, key);
    c.ws();
    if (!c.lit("null", 4)) {
        has = 1;
        if (!c.eat('{')) c.fail(SC_TRACE_ERR_OUTCOME, key);
        for (int m = 0; m < 2 && !c.code; m++) {
            c.ws();
            if (c.lit("\"termination\"", 13)) {
                c.ws();
                if (!c.eat(':')) c.fail(SC_TRACE_ERR_OUTCOME, key);
                c.ws();
                if (!c.eat('"')) c.fail(SC_TRACE_ERR_OUTCOME, key);
                char name[24];
                int k = 0;
                for (int ch = c.peek(); k < 23 && ch != '"' && ch >= 0; ch = c.peek()) name[k++] = (char)ch, c.i++;
                name[k] = 0;
                if (!c.eat('"')) c.fail(SC_TRACE_ERR_OUTCOME, key);
                for (int t = 1; t <= 10 && !term; t++) {
                    int j = 0;
                    while (j <= k && TERM_NAMES[t][j] == name[j]) j++;
                    if (j == k + 1) term = t;
                }
                if (!term) c.fail(SC_TRACE_ERR_OUTCOME, key);
            } else if (c.lit("\"winner\"", 8)) {
                c.ws();
                if (!c.eat(':')) c.fail(SC_TRACE_ERR_OUTCOME, key);
                c.ws();
                if (c.lit("null", 4)) winner = -1;
                else if (c.lit("\"White\"", 7)) winner = 1;
                else if (c.lit("\"Black\"", 7)) winner = 0;
                else c.fail(SC_TRACE_ERR_OUTCOME, key);
            } else {
                c.fail(SC_TRACE_ERR_OUTCOME, key);
            }
            c.ws();
            if (m == 0 && !c.eat(',')) c.fail(SC_TRACE_ERR_OUTCOME, key);
        }
        if (!c.eat('}') || !term || winner == -2) c.fail(SC_TRACE_ERR_OUTCOME, key);
    }
    out[0] = has;
    out[1] = has ? term : 0;
    out[2] = has ? winner : -1;
}

// the last non-white byte in front of offset q (-1: none), over at most MAX_SPACE bytes of white space
__device__ int prev_token_byte(const File& f, uint32_t q, bool* too_long) {
    for (uint32_t k = 1; k <= MAX_SPACE + 1; k++) {
        if (k > q) return -1;
        const int c = f.p[q - k];
        if (!is_ws(c)) return c;
    }
    *too_long = true;
    return -1;
}
__device__ int key_id(const File& f, uint32_t q) {
    Cur c{f, q + 1};
    if (c.lit("steps\"", 6)) return K_STEPS;
    if (c.lit("outcome\"", 8)) return K_OUTCOME;
    if (c.lit("opening\"", 8)) return K_OPENING;
    if (c.lit("fen\"", 4)) return K_FEN;
    return K_OTHER;
}

// the running numbers of a file: steps, children, opening moves, "steps" keys, and the children since the last step (a
// segmented sum: a step restarts it)
struct Cnt {
    uint32_t steps, child, open, keys, since;
};
struct CntOp {
    __device__ __forceinline__ Cnt operator()(const Cnt& a, const Cnt& b) const {
        return {a.steps + b.steps, a.child + b.child, a.open + b.open, a.keys + b.keys, b.steps ? b.since : a.since + b.since};
    }
};
struct SumOp {
    __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; }
};
struct MaxOp {
    __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; }
};
__device__ __forceinline__ uint32_t lane_up(uint32_t v, int o) { return __shfl_up(v, o, 64); }
__device__ __forceinline__ Cnt lane_up(const Cnt& v, int o) {
    return {__shfl_up(v.steps, o, 64), __shfl_up(v.child, o, 64), __shfl_up(v.open, o, 64), __shfl_up(v.keys, o, 64), __shfl_up(v.since, o, 64)};
}
// exclusive scan over the 256 threads of the workgroup and the total: shuffles inside each wavefront, the four wave totals
// through s_w[4].  One barrier: the caller does not touch s_w again before another barrier has passed.
template <class T, class Op>
__device__ __forceinline__ T block_scan(T v, T ident, Op op, T* s_w, T* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T x = lane_up(inc, o);
        if (lane >= o) inc = op(x, inc);
    }
    if (lane == 63) s_w[w] = inc;
    T ex = lane_up(inc, 1);
    if (lane == 0) ex = ident;
    __syncthreads();
    T pre = ident, tot = ident;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const T t = s_w[k];
        if (k < w) pre = op(pre, t);
        tot = op(tot, t);
    }
    *total = tot;
    return op(pre, ex);
}

__device__ __forceinline__ void report(unsigned long long* s_err, int code, uint32_t at) {
    atomicMin(s_err, ((unsigned long long)at << 8) | (unsigned)code);
}

template <bool EMIT>
__global__ __launch_bounds__(256, 2) void k_trace(Text T, Files F, Packed P) {   // (two workgroups per CU: at most 256 VGPRs)
    const int g = blockIdx.x, tid = threadIdx.x;
    __shared__ unsigned long long s_err;
    __shared__ int s_top, s_has_fen, s_outcome[3];
    __shared__ uint32_t s_q[4], s_d[4], s_k[4];
    __shared__ Cnt s_c[4];
    if (g >= T.n) return;
    if (EMIT && F.status[g] != 0) return;   // (the whole workgroup)
    const uint64_t o0 = T.off[g];
    __shared__ uint4 s_text[2][WINDOW / 16];   // two windows in turn: a thread still reading one is at most one barrier behind
    File f{reinterpret_cast<const unsigned char*>(T.text) + o0, (uint32_t)(T.off[g + 1] - o0), nullptr, 0};
    const uint32_t mis = (uint32_t)(o0 & 15);
    const unsigned char* const grid = f.p - mis;   // 16-byte aligned, inside the buffer
    const uint64_t n_chunks = ((uint64_t)mis + f.len + CHUNK - 1) / CHUNK;
    const uint32_t mb = EMIT ? P.step_base[g] : 0, cb = EMIT ? P.child_base[g] : 0, ob = EMIT ? P.open_base[g] : 0;
    if (tid == 0) {
        s_err = ~0ull;
        s_top = 0;
        s_has_fen = 0;
        s_outcome[0] = 0, s_outcome[1] = 0, s_outcome[2] = -1;
    }
    __syncthreads();
    uint32_t carry_q = 0, carry_d = 0, carry_key = K_OTHER;
    Cnt carry{0, 0, 0, 0, 0};
    for (uint64_t ch = 0; ch < n_chunks; ch++) {
        const uint64_t gpos = ch * CHUNK + (uint64_t)tid * 16;   // on the grid
        const int64_t r0 = (int64_t)gpos - mis;                  // in the file: of the thread's first byte
        unsigned char b[16];
        uint4* const window = s_text[ch & 1];
        if (tid < (int)(AHEAD / 16) && gpos + CHUNK < (uint64_t)mis + f.len)
            window[CHUNK / 16 + tid] = *reinterpret_cast<const uint4*>(grid + gpos + CHUNK);
        f.win = reinterpret_cast<const unsigned char*>(window);
        f.win0 = (uint32_t)(ch * CHUNK) - mis;
        if (r0 + 15 >= 0 && r0 < (int64_t)f.len) {
            const uint4 w = *reinterpret_cast<const uint4*>(grid + gpos);
            window[tid] = w;   // (visible to the owners behind the barriers of the scans)
            const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int64_t r = r0 + k;
                b[k] = (r >= 0 && r < (int64_t)f.len) ? (unsigned char)(ws[k >> 2] >> (8 * (k & 3))) : (unsigned char)' ';
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; k++) b[k] = ' ';
        }
        const uint32_t at0 = (uint32_t)r0;   // (+ k: the offset of byte k wherever that byte is inside the file)

        // 1. strings
        uint32_t quotes = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) quotes |= (uint32_t)(b[k] == '"') << k;
        uint32_t tq;
        uint32_t in = (carry_q + block_scan((uint32_t)__popc(quotes), 0u, SumOp{}, s_q, &tq)) & 1u;
        carry_q += tq;
        uint32_t outside = 0, openq = 0, esc = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            if ((quotes >> k) & 1u) {
                if (!in) openq |= 1u << k;
                in ^= 1u;
            } else if (!in) {
                outside |= 1u << k;
            } else if (b[k] == '\\') {
                esc |= 1u << k;
            }
        }
        if (!EMIT && esc) report(&s_err, SC_TRACE_ERR_ESCAPE, at0 + (uint32_t)__ffs(esc) - 1u);
        // 2. depth (modulo 2^32: a text that closes more than it opens is refused below)
        uint32_t delta = 0;
#pragma unroll
        for (int k = 0; k < 16; k++)
            if ((outside >> k) & 1u) delta += (uint32_t)(b[k] == '[' || b[k] == '{') - (uint32_t)(b[k] == ']' || b[k] == '}');
        uint32_t td;
        const int d0 = (int)(carry_d + block_scan(delta, 0u, SumOp{}, s_d, &td));
        carry_d += td;
        // 3. the keys of the top object, and what only the depth tells
        uint32_t top_str = 0, stray = 0;   // strings in the top object; bytes that belong nowhere
        int d = d0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int c = b[k];
            if ((openq >> k) & 1u) {
                if (d == 1) top_str |= 1u << k;
            } else if ((outside >> k) & 1u) {
                if (c == '[' || c == '{') {
                    if (d == 0) {
                        if (c == '{') s_top = 1;
                        else stray |= 1u << k;
                    }
                    d++;
                } else if (c == ']' || c == '}') {
                    d--;
                    if (d < 0) stray |= 1u << k;
                } else if (d == 0 && !is_ws(c)) {
                    stray |= 1u << k;
                }
            }
        }
        if (!EMIT && stray) report(&s_err, SC_TRACE_ERR_UNBALANCED, at0 + (uint32_t)__ffs(stray) - 1u);
        uint64_t key_at = 0;    // a nibble per byte: key id + 1
        uint32_t last_key = 0;  // (position in the chunk + 1) << 3 | id
        for (uint32_t m = top_str; m; m &= m - 1) {
            const int k = __ffs(m) - 1;
            bool too_long = false;
            const int pc = prev_token_byte(f, at0 + k, &too_long);
            if (too_long) {
                if (!EMIT) report(&s_err, SC_TRACE_ERR_SPACE, at0 + k - (MAX_SPACE + 1));
            } else if (pc == '{' || pc == ',') {
                const int id = key_id(f, at0 + k);
                key_at |= (uint64_t)(id + 1) << (4 * k);
                last_key = ((uint32_t)(tid * 16 + k + 1) << 3) | (uint32_t)id;
            }
        }
        uint32_t tk;
        const uint32_t ek = block_scan(last_key, 0u, MaxOp{}, s_k, &tk);
        int key = ek ? (int)(ek & 7u) : (int)carry_key;
        if (tk) carry_key = tk & 7u;
        // 4. events
        uint64_t ev_at = 0;   // a nibble per byte: Ev
        Cnt mine{0, 0, 0, 0, 0};
        d = d0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int c = b[k];
            int ev = EV_NONE;
            if ((openq >> k) & 1u) {
                if (d == 1) {
                    const int nib = (int)((key_at >> (4 * k)) & 15u);
                    if (nib) {
                        key = nib - 1;
                        if (key == K_STEPS) ev = EV_KEY_STEPS, mine.keys++;
                        else if (key == K_OUTCOME) ev = EV_KEY_OUTCOME;
                    } else if (key == K_FEN) {
                        ev = EV_FEN;
                    }
                } else if (d == 2 && key == K_OPENING) {
                    ev = EV_OPEN_MOVE, mine.open++;
                }
            } else if ((outside >> k) & 1u) {
                if (c == '[' || c == '{') {
                    d++;
                    if (c == '[' && key == K_STEPS) {
                        if (d == 3) ev = EV_STEP, mine.steps++, mine.since = 0;
                        else if (d == 5) ev = EV_CHILD, mine.child++, mine.since++;
                        else if (d == 2 || d == 4) ev = EV_NEED_ARR_OR_CLOSE;
                    } else if (c == '[' && key == K_OPENING && d == 2) {
                        ev = EV_NEED_STR_OR_CLOSE;
                    }
                } else if (c == ']' || c == '}') {
                    d--;
                    if (c == ']' && key == K_STEPS && d == 3) ev = EV_NEED_CLOSE;
                } else if (c == ',') {
                    if (key == K_STEPS && (d == 2 || d == 4)) ev = EV_NEED_ARR;
                    else if (key == K_OPENING && d == 2) ev = EV_NEED_STR;
                }
            }
            ev_at |= (uint64_t)ev << (4 * k);
        }
        Cnt tc;
        Cnt run = CntOp{}(carry, block_scan(mine, Cnt{0, 0, 0, 0, 0}, CntOp{}, s_c, &tc));
        carry = CntOp{}(carry, tc);
        // 5. the owners' work: every thread takes its own events in turn (not the 16 byte positions in turn: the lanes of a
        // wavefront then read side by side), and events that begin alike share their first steps
        for (uint64_t m = ev_at; m;) {
            const int k = (__ffsll((unsigned long long)m) - 1) >> 2;
            const int ev = (int)((m >> (4 * k)) & 15u);
            m &= ~(15ull << (4 * k));
            const bool elem = ev == EV_STEP || ev == EV_CHILD;
            if (EMIT && !elem && ev != EV_OPEN_MOVE) continue;
            const uint32_t at = at0 + k;
            Cur c{f, at};
            int x = 0;
            uint16_t mv = 0;
            if (elem || ev >= EV_NEED_ARR_OR_CLOSE) {   // behind a bracket or a comma: the next token
                c.i++;
                c.ws();
                x = c.peek();
            }
            if (elem) {   // [move, ...: up to the second element
                if (x != '"') c.fail(SC_TRACE_ERR_SHAPE, at);
                mv = c.move();
                c.ws();
                if (!c.eat(',')) c.fail(SC_TRACE_ERR_SHAPE, c.i);
                c.ws();
            }
            switch (ev) {
            case EV_STEP:
                if (EMIT) {
                    P.moves[mb + run.steps] = mv;
                    P.child_off[mb + run.steps] = cb + run.child;
                } else {
                    if (run.steps >= MAX_PLIES) report(&s_err, SC_TRACE_ERR_PLIES, at);
                    step_tail(c);
                }
                run.steps++;
                run.since = 0;
                break;
            case EV_CHILD: {
                if (!EMIT && run.since >= MAX_CHILDREN) report(&s_err, SC_TRACE_ERR_CHILDREN, at);
                const uint32_t count = child_count(c);
                if (EMIT) {
                    P.child_mv[cb + run.child] = mv;
                    P.child_n[cb + run.child] = count;
                }
                run.child++;
                run.since++;
                break;
            }
            case EV_OPEN_MOVE:
                mv = c.move();
                if (EMIT) P.opening[ob + run.open] = mv;
                run.open++;
                break;
            case EV_KEY_STEPS:
                if (run.keys >= 1) c.fail(SC_TRACE_ERR_STEPS, at);
                c.i += 7;
                c.ws();
                if (!c.eat(':')) c.fail(SC_TRACE_ERR_STEPS, at);
                c.ws();
                if (c.peek() != '[') c.fail(SC_TRACE_ERR_STEPS, at);
                run.keys++;
                break;
            case EV_KEY_OUTCOME: {
                int oc[3];
                parse_outcome(c, oc);
                if (!c.code) s_outcome[0] = oc[0], s_outcome[1] = oc[1], s_outcome[2] = oc[2];
                break;
            }
            case EV_FEN: {
                char* out = F.fen + (size_t)g * FEN_CAP;
                int n = 0, y;
                while ((y = f.at(at + 1 + (uint32_t)n)) != '"' && y >= 0 && n < FEN_CAP - 1) out[n++] = (char)y;
                out[n] = 0;
                if (y != '"') c.fail(SC_TRACE_ERR_SHAPE, at);
                else s_has_fen = 1;
                break;
            }
            default: {
                const bool ok = ev == EV_NEED_ARR_OR_CLOSE ? (x == '[' || x == ']') : ev == EV_NEED_ARR ? x == '[' : ev == EV_NEED_CLOSE ? x == ']'
                                : ev == EV_NEED_STR_OR_CLOSE ? (x == '"' || x == ']') : x == '"';
                if (!ok) c.fail(SC_TRACE_ERR_SHAPE, at);
                break;
            }
            }
            if (!EMIT && c.code) report(&s_err, c.code, c.where);
        }
    }
    if (EMIT) return;
    __syncthreads();
    if (tid == 0) {
        unsigned long long e = s_err;
        const unsigned long long end = (unsigned long long)f.len << 8;
        if ((carry_q & 1u) || carry_d != 0 || !s_top) e = e < (end | SC_TRACE_ERR_UNBALANCED) ? e : (end | SC_TRACE_ERR_UNBALANCED);
        if (carry.keys == 0) e = e < (end | SC_TRACE_ERR_STEPS) ? e : (end | SC_TRACE_ERR_STEPS);
        const bool ok = e == ~0ull;
        F.status[g] = ok ? 0 : -(int32_t)(e & 255u);
        F.err_at[g] = ok ? 0u : (uint32_t)(e >> 8);
        F.n_steps[g] = ok ? carry.steps : 0u;
        F.n_children[g] = ok ? carry.child : 0u;
        F.n_opening[g] = ok ? carry.open : 0u;
        F.outcome[g * 3 + 0] = ok ? s_outcome[0] : 0;
        F.outcome[g * 3 + 1] = ok ? s_outcome[1] : 0;
        F.outcome[g * 3 + 2] = ok ? s_outcome[2] : -1;
        F.has_fen[g] = ok ? s_has_fen : 0;
        if (!ok || !s_has_fen) F.fen[(size_t)g * FEN_CAP] = 0;
    }
}

// the codes of sc_traces_encode_device that the reader decides, over the encoder's: over[g] != 0 wins
__global__ __launch_bounds__(256) void k_trace_status(int n, const int32_t* __restrict__ over, int32_t* __restrict__ status) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n && over[g] != 0) status[g] = over[g];
}

}  // namespace sctr

namespace scl {
void trace_count(const sctr::Text& t, const sctr::Files& f, hipStream_t s) {
    if (t.n <= 0) return;
    hipLaunchKernelGGL(sctr::k_trace<false>, dim3(t.n), dim3(256), 0, s, t, f, sctr::Packed{});
}
void trace_emit(const sctr::Text& t, const sctr::Files& f, const sctr::Packed& p, hipStream_t s) {
    if (t.n <= 0) return;
    hipLaunchKernelGGL(sctr::k_trace<true>, dim3(t.n), dim3(256), 0, s, t, f, p);
}
void trace_status(int n, const int32_t* d_over, int32_t* d_status, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(sctr::k_trace_status, dim3((n + 255) / 256), dim3(256), 0, s, n, d_over, d_status);
}
}  // namespace scl
