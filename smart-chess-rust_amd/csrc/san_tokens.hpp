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

}  // namespace scsan
