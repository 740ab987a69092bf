// fen_text_check.cpp -- stand-alone memory-safety check of the FEN reader (csrc/fen_text.cpp), host only:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Ismart-chess-rust_amd/csrc \
//       tools/fen_text_check.cpp smart-chess-rust_amd/csrc/fen_text.cpp -o fen_text_check
//   fen_text_check [FILE ...]
//
// Every FEN of the tests (tests/test_fen_abi.py, tests/test_gpu_fen.py), a set of malformed ones and every line of the given
// files are parsed cut off at EVERY byte offset, each prefix copied into a heap block of exactly its size -- a read past `len` is
// one byte outside the block, which the sanitizer reports.  An accepted prefix is also formatted (fen_format) into heap blocks
// of exactly the text's size + 1, of half of it and of one byte, and the full-size text must parse back into the same fields.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>

#include "fen_text.hpp"

static const char* const TEXTS[] = {
    // the accepted ones
    "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1",
    "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1",
    "8/2p5/3p4/KP5r/1R3p1k/8/4P1P1/8 w - - 0 1",
    "r3k2r/Pppp1ppp/1b3nbN/nP6/BBP1P3/q4N2/Pp1P2PP/R2Q1RK1 w kq - 0 1",
    "rnbq1k1r/pp1Pbppp/2p5/8/2B5/8/PPP1NnPP/RNBQK2R w KQ - 1 8",
    "r4rk1/1pp1qppp/p1np1n2/2b1p1B1/2B1P1b1/P1NP1N2/1PP1QPPP/R4RK1 w - - 0 10",
    "1k1r4/1r5p/p4n1P/1ppP1P2/PP6/4PP1b/3B4/R1N1K3 b - - 0 39",
    "r1bqkbnr/pppp1ppp/2n5/4p2Q/2B1P3/8/PPPP1PPP/RNB1K1NR w KQkq - bm Qxf7+; id \"scholar\";",
    "rnbqkbnr/ppp1p1pp/8/3pPp2/8/8/PPPP1PPP/RNBQKBNR w KQkq f6 0 3",
    "8/8/8/8/8/8/4K3/4k3 w - - 0 1",
    "4k3/8/8/8/8/8/8/4K3 w - - 0 1",
    "7k/5Q2/6K1/8/8/8/8/8 b - - 0 1",
    "4k3/8/8/8/8/8/4P3/4K3 w - - 100 80",
    "4k3/8/8/8/8/8/4P3/4K2R w K - 99 80",
    "4k3/8/8/8/4P3/8/8/4K3 b - e3 0 1",
    "QQQQQQQQ/Q7/8/8/8/PPPPPPPP/8/K6k w - - 0 1",
    "3P4/8/8/8/8/8/8/K6k w - - 0 1",
    "8/8/8/8/8/8/8/K7 w - - 0 1",
    "  rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR\tb\tKq\ta3\t12\t0\n",
    // the malformed ones
    "",
    "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP w KQkq - 0 1",
    "rnbqkbnr/pppppppp/9/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1",
    "rnbqkbnr/pppppppp/44/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1",
    "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNx w KQkq - 0 1",
    "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR W KQkq - 0 1",
    "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkqK - 0 1",
    "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w HAha - 0 1",
    "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq e4 0 1",
    "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - -1 1",
    "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 70000",
    "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 99999999999999999999 1",
    "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR/8 w KQkq - 0 1",
    "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNRR w qK - 0 1",
    "\xff\xfe/\x80 w \x01 -",
    "////////////////////////////////////////////////////////////////////////////////",
    "8888888888888888888888888888888888888888888888888888888888888888888888888888888",
};

static size_t check(const std::string& text) {
    size_t calls = 0;
    for (size_t len = 0; len <= text.size(); len++) {
        char* t = static_cast<char*>(malloc(len ? len : 1));
        memcpy(t, text.data(), len);
        sc_fen_fields f;
        const int rc = scfen::fen_parse(len ? t : nullptr, len, &f);
        calls++;
        if (rc > 0 || rc < -6) {
            fprintf(stderr, "code %d from %zu bytes\n", rc, len);
            exit(1);
        }
        if (rc == 0) {
            char one[1];
            const int n = scfen::fen_format(&f, true, one, 1);
            for (int cap : {n + 1, n / 2, 1}) {
                char* out = static_cast<char*>(malloc((size_t)cap));
                if (scfen::fen_format(&f, true, out, cap) != n || strlen(out) != (size_t)(cap > n ? n : cap - 1)) {
                    fprintf(stderr, "fen_format: the length depends on cap (%zu bytes)\n", len);
                    exit(1);
                }
                if (cap == n + 1) {
                    sc_fen_fields g;
                    if (scfen::fen_parse(out, (size_t)n, &g) != 0 || memcmp(&f, &g, sizeof f) != 0) {
                        fprintf(stderr, "'%s' does not parse back into its fields\n", out);
                        exit(1);
                    }
                    calls++;
                }
                free(out);
            }
        }
        free(t);
    }
    return calls;
}

int main(int argc, char** argv) {
    size_t texts = 0, calls = 0;
    for (const char* h : TEXTS) {
        calls += check(h);
        texts++;
    }
    calls += check(std::string("8/8/8/8/8/8/4K3/4k3 w\0- - 0 1", 28));   // a zero byte is no white space
    texts++;
    for (int a = 1; a < argc; a++) {
        std::ifstream f(argv[a]);
        if (!f) {
            fprintf(stderr, "cannot read %s\n", argv[a]);
            return 1;
        }
        for (std::string line; std::getline(f, line);) {
            calls += check(line + "\n");
            texts++;
        }
    }
    printf("fen_text_check ok: %zu texts, %zu bounded calls\n", texts, calls);
    return 0;
}
