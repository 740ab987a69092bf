// san_tokens_check.cpp -- stand-alone memory-safety check of the SAN tokenizer (csrc/san_tokens.cpp), host only:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Ismart-chess-rust_amd/csrc \
//       tools/san_tokens_check.cpp smart-chess-rust_amd/csrc/san_tokens.cpp -o san_tokens_check
//   san_tokens_check tests/golden/ref_sample_games.csv
//
// Every line of the given files (a CSV row holds one game's movetext among its columns: the other columns are just more text)
// and a set of hand-written movetexts are tokenized cut off at EVERY byte offset, each prefix copied into a heap block of exactly
// its size and the tokens written into heap blocks of exactly `cap` entries -- a read past `len` or a write past `cap` is one
// byte outside a block, which the sanitizer reports.  Three calls per prefix: the count query (cap 0), the exact cap, half of it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "san_tokens.hpp"

static const char* const HAND[] = {
    "",
    "1. e4 e5 2. Nf3 Nc6 3. Bb5 a6 1-0",
    "1.e4 e5 2.Nf3 2...Nc6 3. ... Bb5 12",
    "1. e4 {best by test} e5 (1... c5 (1... e6 {the ) French} 2. d4) 2. Nf3) 2. Nf3 $1 Nc6 $14 ; Bb5 is next\n3. Bb5 a6 *",
    "e4 {never closed e5",
    "e4 (never (closed {e5",
    "[Event \"a ] in \\\" a value\"]\n[Site \"?\"] 1. d4 d5 1/2-1/2",
    "[Event \"never closed",
    "Nf3!?+ Qxf7#!! e8=Q+ exd8=N# O-O+ O-O-O# 0-0 0-0-0 e4?? ! 0-1",
    "1. e4 Ng1xf3=Q 2. d4 ) } d5 Qa1xh8+ abcdefghijklmnopqrstuvwxyz",
    "\xff\xfe\x80 e4 \x01\x02",
};

static size_t check(const std::string& text) {
    size_t calls = 0;
    for (size_t len = 0; len <= text.size(); len++) {
        char* t = static_cast<char*>(malloc(len ? len : 1));
        memcpy(t, text.data(), len);
        const size_t n = scsan::san_tokenize(len ? t : nullptr, len, nullptr, 0);
        if (n > len) {   // every token takes a byte of text at least
            fprintf(stderr, "%zu tokens from %zu bytes\n", n, len);
            exit(1);
        }
        for (size_t cap : {n, n / 2}) {
            uint64_t* out = static_cast<uint64_t*>(malloc(cap ? cap * 8 : 1));
            if (scsan::san_tokenize(t, len, cap ? out : nullptr, cap) != n) {
                fprintf(stderr, "the count depends on cap (%zu bytes)\n", len);
                exit(1);
            }
            for (size_t k = 0; k < cap; k++)
                if (out[k] != scsan::TOKEN_RESERVED && (out[k] >> 56)) {
                    fprintf(stderr, "a token of 8 characters (%zu bytes)\n", len);
                    exit(1);
                }
            free(out);
            calls++;
        }
        free(t);
    }
    return calls;
}

int main(int argc, char** argv) {
    size_t texts = 0, calls = 0;
    for (const char* h : HAND) {
        calls += check(h);
        texts++;
    }
    calls += check(std::string("e4\0d4 e5", 8));   // a zero byte separates
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
    printf("san_tokens_check ok: %zu texts, %zu bounded calls\n", texts, calls);
    return 0;
}
