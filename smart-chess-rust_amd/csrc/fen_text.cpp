// fen_text.cpp -- the host reader of FEN / EPD text (fen_text.hpp).  Every read is bounded by `len`: the text need not be
// zero-terminated, and a text cut off anywhere is refused with the code of the field it was cut in (or, past the fourth field,
// read as an EPD record: the clocks are optional).
//
// Grammar: python-chess's Board.set_fen for standard chess.  Fields are separated by runs of white space.
//   board     eight ranks separated by '/', each of digits 1-8 and letters of pnbrqkPNBRQK that sum to 8, no two digits in a row
//   turn      w | b
//   castling  - | up to two of KQ followed by up to two of kq, no letter twice (Shredder / X-FEN file letters are refused)
//   ep        - | [a-h][36]
//   clocks    present when the fifth AND sixth words are integers (-?[0-9]+): halfmove in 0..65535, fullmove in 0..65535 with 0
//             read as 1 (python-chess does the same); anything else behind the fourth field -- EPD operations -- is ignored and
//             the clocks are 0 and 1
#include "fen_text.hpp"

#include <string.h>

namespace scfen {
namespace {

inline bool is_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; }

struct Words {
    const char* t;
    size_t len, i;
    // the next word: [*w, *w + *n); false at the end of the text
    bool next(const char** w, size_t* n) {
        while (i < len && is_space(t[i])) i++;
        if (i >= len) return false;
        const size_t b = i;
        while (i < len && !is_space(t[i])) i++;
        *w = t + b;
        *n = i - b;
        return true;
    }
};

int piece_index(char lower) {
    switch (lower) {
        case 'p': return 0;
        case 'n': return 1;
        case 'b': return 2;
        case 'r': return 3;
        case 'q': return 4;
        case 'k': return 5;
        default: return -1;
    }
}

bool parse_board(const char* w, size_t n, sc_fen_fields* out) {
    int rank = 7, file = 0;
    bool prev_digit = false;
    for (size_t k = 0; k < n; k++) {
        const char c = w[k];
        if (c == '/') {
            if (file != 8 || rank == 0) return false;
            rank--;
            file = 0;
            prev_digit = false;
        } else if (c >= '1' && c <= '8') {
            if (prev_digit) return false;
            file += c - '0';
            if (file > 8) return false;
            prev_digit = true;
        } else {
            const bool white = c >= 'A' && c <= 'Z';
            const int t = piece_index((char)(white ? c + 32 : c));
            if (t < 0 || file > 7) return false;
            const uint64_t b = 1ULL << (rank * 8 + file);
            out->pcs[t] |= b;
            out->occ[white ? 1 : 0] |= b;
            file++;
            prev_digit = false;
        }
    }
    return rank == 0 && file == 8;
}

bool parse_castling(const char* w, size_t n, int32_t* out) {
    if (n == 1 && w[0] == '-') {
        *out = 0;
        return true;
    }
    if (n > 4) return false;
    int bits = 0;
    bool lower_seen = false;
    for (size_t k = 0; k < n; k++) {
        const char c = w[k];
        const int b = c == 'K' ? 1 : c == 'Q' ? 2 : c == 'k' ? 4 : c == 'q' ? 8 : 0;
        if (!b || (bits & b)) return false;
        if (b >= 4) lower_seen = true;
        else if (lower_seen) return false;   // White's letters come first
        bits |= b;
    }
    *out = bits;
    return true;
}

bool is_integer(const char* w, size_t n) {
    size_t k = (n > 0 && w[0] == '-') ? 1 : 0;
    if (k == n) return false;
    for (; k < n; k++)
        if (w[k] < '0' || w[k] > '9') return false;
    return true;
}
// the value of an integer word if it lies in 0..65535, else -1
int32_t clock_value(const char* w, size_t n) {
    if (w[0] == '-') return -1;
    int32_t v = 0;
    for (size_t k = 0; k < n; k++) {
        v = v * 10 + (w[k] - '0');
        if (v > 65535) return -1;
    }
    return v;
}

}  // namespace

void fen_startpos(sc_fen_fields* out) {
    memset(out, 0, sizeof *out);
    out->pcs[0] = 0x00FF00000000FF00ULL;
    out->pcs[1] = 0x4200000000000042ULL;
    out->pcs[2] = 0x2400000000000024ULL;
    out->pcs[3] = 0x8100000000000081ULL;
    out->pcs[4] = 0x0800000000000008ULL;
    out->pcs[5] = 0x1000000000000010ULL;
    out->occ[1] = 0x000000000000FFFFULL;
    out->occ[0] = 0xFFFF000000000000ULL;
    out->turn = 1;
    out->castling = 15;
    out->ep = -1;
    out->halfmove = 0;
    out->fullmove = 1;
}

int fen_parse(const char* text, size_t len, sc_fen_fields* out) {
    sc_fen_fields f;
    memset(&f, 0, sizeof f);
    memset(out, 0, sizeof *out);
    Words ws{text, text ? len : 0, 0};
    const char* w = nullptr;
    size_t n = 0;
    if (!ws.next(&w, &n) || !parse_board(w, n, &f)) return -F_BOARD;
    if (!ws.next(&w, &n) || n != 1 || (w[0] != 'w' && w[0] != 'b')) return -F_TURN;
    f.turn = w[0] == 'w' ? 1 : 0;
    if (!ws.next(&w, &n) || !parse_castling(w, n, &f.castling)) return -F_CASTLING;
    if (!ws.next(&w, &n)) return -F_EP;
    if (n == 1 && w[0] == '-') {
        f.ep = -1;
    } else if (n == 2 && w[0] >= 'a' && w[0] <= 'h' && (w[1] == '3' || w[1] == '6')) {
        f.ep = (w[1] - '1') * 8 + (w[0] - 'a');
    } else {
        return -F_EP;
    }
    f.halfmove = 0;
    f.fullmove = 1;
    const char *w5 = nullptr, *w6 = nullptr;
    size_t n5 = 0, n6 = 0;
    if (ws.next(&w5, &n5) && ws.next(&w6, &n6) && is_integer(w5, n5) && is_integer(w6, n6)) {
        f.halfmove = clock_value(w5, n5);
        if (f.halfmove < 0) return -F_HALFMOVE;
        f.fullmove = clock_value(w6, n6);
        if (f.fullmove < 0) return -F_FULLMOVE;
        if (f.fullmove == 0) f.fullmove = 1;
    }
    *out = f;
    return 0;
}

int fen_format(const sc_fen_fields* f, bool ep_legal, char* buf, int cap) {
    char tmp[112];   // 71 of board at most, 2 turn, 5 castling, 3 ep, 6 + 6 clocks
    int n = 0;
    static const char names[] = "pnbrqk";
    for (int r = 7; r >= 0; r--) {
        int e = 0;
        for (int fl = 0; fl < 8; fl++) {
            const uint64_t b = 1ULL << (r * 8 + fl);
            int t = -1;
            for (int k = 0; k < 6; k++)
                if (f->pcs[k] & b) t = k;
            if (t < 0 || !((f->occ[0] | f->occ[1]) & b)) {
                e++;
                continue;
            }
            if (e) tmp[n++] = (char)('0' + e);
            e = 0;
            tmp[n++] = (char)((f->occ[1] & b) ? names[t] - 32 : names[t]);
        }
        if (e) tmp[n++] = (char)('0' + e);
        if (r) tmp[n++] = '/';
    }
    tmp[n++] = ' ';
    tmp[n++] = f->turn ? 'w' : 'b';
    tmp[n++] = ' ';
    if (!(f->castling & 15)) tmp[n++] = '-';
    if (f->castling & 1) tmp[n++] = 'K';
    if (f->castling & 2) tmp[n++] = 'Q';
    if (f->castling & 4) tmp[n++] = 'k';
    if (f->castling & 8) tmp[n++] = 'q';
    tmp[n++] = ' ';
    if (ep_legal && f->ep >= 0 && f->ep < 64) {
        tmp[n++] = (char)('a' + (f->ep & 7));
        tmp[n++] = (char)('1' + (f->ep >> 3));
    } else {
        tmp[n++] = '-';
    }
    tmp[n++] = ' ';
    for (int k = 0; k < 2; k++) {
        uint32_t v = (uint32_t)(k ? f->fullmove : f->halfmove) & 0xffffu;
        char d[6];
        int nd = 0;
        do {
            d[nd++] = (char)('0' + v % 10);
            v /= 10;
        } while (v);
        while (nd) tmp[n++] = d[--nd];
        if (!k) tmp[n++] = ' ';
    }
    for (int k = 0; k < n && k + 1 < cap; k++) buf[k] = tmp[k];
    if (cap > 0) buf[n < cap ? n : cap - 1] = 0;
    return n;
}

}  // namespace scfen
