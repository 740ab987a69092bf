// san_tokens.hpp -- SAN movetext -> one 8-byte token per half-move (sc_san_tokenize; include/sc_engine.h).  Plain C++, no HIP:
// san_tokens.cpp compiles into the library and into a stand-alone program alike.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace scsan {

// a token: the SAN characters of one half-move, character k in byte k (little-endian), zero-padded, at most 7 of them
constexpr uint64_t TOKEN_RESERVED = ~0ULL;   // "a half-move stands here, but not one that fits a token": malformed on the device

// One game's movetext.  Writes min(count, cap) tokens and returns the count of half-moves in the text (which may exceed cap:
// nothing is written past it).  Skips move numbers (12. / 12... / glued 1.e4), {...} and ;-to-end-of-line comments, nested (...)
// variations, $n NAGs, [...] header tags and lone annotation glyphs; stops at a result (1-0, 0-1, 1/2-1/2, *).  The suffix run
// of + # ! ? is stripped.  Anything else of more than 7 characters, and a stray closing bracket, becomes TOKEN_RESERVED.
size_t san_tokenize(const char* text, size_t len, uint64_t* tokens, size_t cap);

// Tokens -> one line of movetext (sc_san_format): "1. e4 e5 2. Nf3", or with black_first "12... Nf6 13. d4"; a token's
// characters are written as they are (the writer's tokens carry their + / #), a token of 0 ends the text, `result` (or null) is
// appended as a last word.  Returns the length of the whole text; writes at most cap bytes, the final zero among them (cap 0:
// nothing, buf may be null).
size_t san_format(const uint64_t* tokens, size_t n, unsigned fullmove, bool black_first, const char* result, char* buf, size_t cap);

}  // namespace scsan
