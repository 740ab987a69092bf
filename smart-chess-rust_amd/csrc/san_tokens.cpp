// san_tokens.cpp -- the host tokenizer of SAN movetext and its inverse, the formatter (san_tokens.hpp).  Every read of the
// tokenizer is bounded by `len`: the text need not be zero-terminated, and a text cut off anywhere (inside a comment, a variation,
// a tag, a token) ends the game there.  Every write of the formatter is bounded by `cap`.
#include "san_tokens.hpp"

namespace scsan {
namespace {

inline bool is_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f' || c == '\0'; }
inline bool is_digit(char c) { return c >= '0' && c <= '9'; }
inline bool is_suffix(char c) { return c == '+' || c == '#' || c == '!' || c == '?'; }
inline bool ends_word(char c) { return is_space(c) || c == '{' || c == '}' || c == '(' || c == ')' || c == ';'; }

inline bool equals(const char* w, size_t n, const char* lit) {
    size_t k = 0;
    for (; k < n && lit[k]; k++)
        if (w[k] != lit[k]) return false;
    return k == n && !lit[k];
}
inline bool is_result(const char* w, size_t n) { return equals(w, n, "1-0") || equals(w, n, "0-1") || equals(w, n, "1/2-1/2") || equals(w, n, "*"); }

// i: at the '{'; -> behind the closing '}' (or len)
size_t skip_brace(const char* t, size_t len, size_t i) {
    while (i < len && t[i] != '}') i++;
    return i < len ? i + 1 : len;
}
size_t skip_line(const char* t, size_t len, size_t i) {
    while (i < len && t[i] != '\n') i++;
    return i;
}

}  // namespace

size_t san_tokenize(const char* t, size_t len, uint64_t* tokens, size_t cap) {
    size_t n = 0, i = 0;
    auto emit = [&](uint64_t v) {
        if (n < cap) tokens[n] = v;
        n++;
    };
    while (i < len) {
        const char c = t[i];
        if (is_space(c)) {
            i++;
        } else if (c == '{') {
            i = skip_brace(t, len, i);
        } else if (c == ';') {
            i = skip_line(t, len, i);
        } else if (c == '(') {   // a variation: to its closing bracket, comments inside it are opaque
            size_t depth = 0;
            while (i < len) {
                if (t[i] == '{') {
                    i = skip_brace(t, len, i);
                    continue;
                }
                if (t[i] == ';') {
                    i = skip_line(t, len, i);
                    continue;
                }
                if (t[i] == '(') depth++;
                if (t[i] == ')' && --depth == 0) {
                    i++;
                    break;
                }
                i++;
            }
        } else if (c == '[') {   // a header tag: to its ']', which a quoted value may hold too
            bool quoted = false;
            for (i++; i < len; i++) {
                if (quoted && t[i] == '\\' && i + 1 < len) i++;
                else if (t[i] == '"') quoted = !quoted;
                else if (t[i] == ']' && !quoted) break;
            }
            if (i < len) i++;
        } else if (c == ')' || c == '}') {   // closes nothing
            emit(TOKEN_RESERVED);
            i++;
        } else {
            size_t e = i;
            while (e < len && !ends_word(t[e])) e++;
            const char* w = t + i;
            size_t wn = e - i;
            i = e;
            if (is_result(w, wn)) break;
            if (w[0] == '$') continue;
            // a move number: digits and the dots behind them, alone or glued to the move; dots alone ("1. ... e5") too
            size_t k = 0;
            while (k < wn && is_digit(w[k])) k++;
            if (k == wn) continue;
            if (w[k] == '.') {
                while (k < wn && w[k] == '.') k++;
                w += k;
                wn -= k;
                if (wn == 0) continue;
                if (is_result(w, wn)) break;
            }
            while (wn > 0 && is_suffix(w[wn - 1])) wn--;
            if (wn == 0) continue;   // an annotation glyph on its own
            if (wn > 7) {
                emit(TOKEN_RESERVED);
                continue;
            }
            uint64_t v = 0;
            for (size_t b = 0; b < wn; b++) v |= (uint64_t)(unsigned char)w[b] << (8 * b);
            emit(v);
        }
    }
    return n;
}

size_t san_format(const uint64_t* tokens, size_t n, unsigned fullmove, bool black_first, const char* result, char* buf, size_t cap) {
    size_t len = 0;
    auto put = [&](char c) {
        if (len + 1 < cap) buf[len] = c;   // (the last byte is the final zero's)
        len++;
    };
    bool black = black_first;
    for (size_t i = 0; i < n && tokens[i]; i++) {
        if (len) put(' ');
        if (!black || i == 0) {
            char d[12];
            int k = 0;
            for (unsigned v = fullmove; k == 0 || v; v /= 10) d[k++] = (char)('0' + v % 10);
            while (k) put(d[--k]);
            put('.');
            if (black) {
                put('.');
                put('.');
            }
            put(' ');
        }
        for (int b = 0; b < 8; b++) {
            const char c = (char)((tokens[i] >> (8 * b)) & 0xff);
            if (!c) break;
            put(c);
        }
        if (black) fullmove++;
        black = !black;
    }
    if (result && *result) {
        if (len) put(' ');
        for (; *result; result++) put(*result);
    }
    if (cap) buf[len < cap ? len : cap - 1] = 0;
    return len;
}

}  // namespace scsan
