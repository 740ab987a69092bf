// san_format_check.cpp -- stand-alone memory-safety check of the movetext formatter (csrc/san_tokens.cpp), host only:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Ismart-chess-rust_amd/csrc \
//       tools/san_format_check.cpp smart-chess-rust_amd/csrc/san_tokens.cpp -o san_format_check
//   san_format_check tests/golden/ref_sample_games.csv
//
// Hand-written movetexts and every line of the given files are tokenized, and the tokens -- in a heap block of exactly their
// size -- are formatted from White's and from Black's side, with and without a result word, at EVERY cap from 0 to length + 1,
// each into a heap block of exactly `cap` bytes: a write past `cap` is one byte outside a block, which the sanitizer reports.
// Checked besides: the length does not depend on cap, the text written is the terminated prefix of the whole text, and the whole
// text tokenizes back to the tokens it was made of.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "san_tokens.hpp"

static const char* const HAND[] = {
    "",
    "e4",
    "1. e4 e5 2. Nf3 Nc6 3. Bb5 a6",
    "Qh4xe1+ exd8=Q# O-O-O+ O-O Nbd2 R1e2 e8=N",
    "1. e4 e5 2. Nf3 abcdefghijklmnopqrstuvwxyz 3. d4",   // the reserved value: eight 0xff characters
};

static void die(const char* what, const std::string& text) {
    fprintf(stderr, "%s: %s\n", what, text.c_str());
    exit(1);
}

static size_t check(const std::string& text) {
    const size_t n = scsan::san_tokenize(text.data(), text.size(), nullptr, 0);
    uint64_t* tok = static_cast<uint64_t*>(malloc(n ? n * 8 : 1));
    scsan::san_tokenize(text.data(), text.size(), tok, n);
    size_t calls = 0;
    for (int variant = 0; variant < 4; variant++) {
        const bool black_first = variant & 1;
        const char* result = (variant & 2) ? "1/2-1/2" : nullptr;
        const unsigned fullmove = black_first ? 4294967295u : 1u;   // (the longest number too: it wraps around to 0)
        const size_t len = scsan::san_format(n ? tok : nullptr, n, fullmove, black_first, result, nullptr, 0);
        char* whole = static_cast<char*>(malloc(len + 1));
        if (scsan::san_format(tok, n, fullmove, black_first, result, whole, len + 1) != len || strlen(whole) != len) die("length", text);
        for (size_t cap = 0; cap <= len + 1; cap++) {
            char* buf = static_cast<char*>(malloc(cap ? cap : 1));
            if (scsan::san_format(tok, n, fullmove, black_first, result, cap ? buf : nullptr, cap) != len) die("the length depends on cap", text);
            if (cap && (strlen(buf) != cap - 1 || memcmp(buf, whole, cap - 1) != 0)) die("not the terminated prefix", text);
            free(buf);
            calls++;
        }
        // the tokenizer strips suffixes and stops at the result: compare through it
        std::vector<uint64_t> back(n + 1), plain(n + 1);
        const size_t nb = scsan::san_tokenize(whole, len, back.data(), n + 1);
        std::string bare;
        for (size_t k = 0; k < n; k++) {
            for (int b = 0; b < 8 && ((tok[k] >> (8 * b)) & 0xff); b++) bare += (char)((tok[k] >> (8 * b)) & 0xff);
            bare += ' ';
        }
        const size_t np = scsan::san_tokenize(bare.data(), bare.size(), plain.data(), n + 1);
        if (nb != np || memcmp(back.data(), plain.data(), nb * 8) != 0) die("the text does not read back", text);
        free(whole);
    }
    free(tok);
    return calls;
}

int main(int argc, char** argv) {
    size_t texts = 0, calls = 0;
    for (const char* h : HAND) {
        calls += check(h);
        texts++;
    }
    {   // a token of 0 ends the text
        const uint64_t t[3] = {0x3465, 0, 0x3565};
        char buf[16];
        if (scsan::san_format(t, 3, 1, false, nullptr, buf, sizeof buf) != 5 || strcmp(buf, "1. e4") != 0) die("a zero token", "e4 0 e5");
    }
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
    printf("san_format_check ok: %zu texts, %zu bounded calls\n", texts, calls);
    return 0;
}
