// fen_text.hpp -- FEN / EPD text -> the raw fields of a position (sc_fen_parse; include/sc_engine.h).  Plain C++, no HIP and no
// rules code: fen_text.cpp compiles into the library and into a stand-alone program alike.  Whether the position can be played
// is decided on the device (fen_kernels.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/sc_engine.h"

namespace scfen {

// the failing field of a refused text: sc_fen_parse returns its negative
enum { F_BOARD = 1, F_TURN = 2, F_CASTLING = 3, F_EP = 4, F_HALFMOVE = 5, F_FULLMOVE = 6 };

// Every read is bounded by len.  Returns 0 and fills *out, or -(failing field) and leaves *out zeroed.
int fen_parse(const char* text, size_t len, sc_fen_fields* out);

// the fields of the start position
void fen_startpos(sc_fen_fields* out);

// python-chess Board.fen() of the fields: the ep square is printed only with ep_legal (a legal en-passant capture exists).
// Writes at most cap bytes including the final zero; returns the length of the whole text (it needs cap > that).
int fen_format(const sc_fen_fields* f, bool ep_legal, char* buf, int cap);

}  // namespace scfen
