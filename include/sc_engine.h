/*
 * sc_engine.h -- C ABI of libsc_engine.so, the MI355X-native drop-in for the MCTS + NN rollout
 * hot path of pierric/smart-chess-rust.
 *
 * Plain pointers and sizes only (no torch / C++ types).  Every entry point returns 0 on success
 * and a negative code on failure; sc_last_error() gives the thread-local message.  Nothing aborts
 * across the ABI (the reference unwrap()s/panics instead: src/backends/torch.rs:27-31,100,111).
 * A handle is bound to one GPU and must be driven by one host thread at a time; distinct handles
 * (one per GPU) are independent -- this is how games shard over the 8 GPUs of a node.
 *
 * Two levels, as laid out in SURVEY.md section 8(b):
 *
 *  L-predict  -- the reference's `trait Game<S>::predict` contract (src/game.rs:3-15) as
 *                implemented by src/backends/torch.rs:89-146 / src/backends/onnx.rs:14-56,
 *                batched.  The reference-side binding is a `impl Game<BoardState> for ChessHip`
 *                (INTEGRATION.md).
 *  L-search   -- the whole per-game loop of src/main.rs:155-238 (mcts::mcts src/mcts.rs:237-289,
 *                mcts::step :292-328, Trace src/trace.rs:5-42) for many concurrent games on one GPU.
 *
 * Layout conventions (identical to the reference's post-_encode tensors):
 *   boards : int8  [n][8][8][112]  (rank, file, plane)      src/chess.rs:828-842, :845-877
 *   meta   : int32 [n][7]                                    src/chess.rs:652-662
 *   moves  : uint16 = from | to<<6 | promo<<12, squares a1=0..h8=63, promo in python-chess piece
 *            types (0 none, 2 N, 3 B, 4 R, 5 Q); castling is the king's two-square move (e1g1)
 *   action index: rank*584 + file*73 + type after rotating Black's moves (src/chess.rs:504-551)
 */
#ifndef SC_ENGINE_H
#define SC_ENGINE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SC_MAX_MOVES 224      /* row stride of per-position move tables (218 is the chess maximum) */
#define SC_POLICY_SIZE 4672   /* 8*8*73 */
#define SC_BOARD_BYTES 7168   /* 8*8*112 */

typedef struct sc_engine sc_engine;
typedef struct sc_selfplay sc_selfplay;

const char* sc_last_error(void);
/* Return codes (every entry point: 0 = ok, or a small positive "not yet / not there" code where its comment says so):
 *   -1 bad argument or request, -2 HIP runtime error, -3 no GPU (there is no CPU fallback),
 *   SC_ERR_HANDOFF: the self-play handle is POISONED -- an internal hand-off of one of its step launches timed out
 *   (sc_selfplay_stats.error_flags & 48), so values were computed from stale data and its trees / traces are invalid.  Once the
 *   host has seen that (any synchronising call), sc_selfplay_enqueue_sims / _enqueue_interleaved / _run / _synchronize / _poll /
 *   _get_trace / _write_trace_json refuse with this code; sc_selfplay_get_stats still answers (the flags).  Destroy the handle;
 *   handles created afterwards on that device use the two-launch step, which has no hand-off between workgroups. */
#define SC_ERR_HANDOFF (-5)
#define SC_ERR_CAPACITY (-4)   /* sc_san_tokenize: the token buffer is too small */
int sc_device_count(void);
/* Launch-path state of the HIP runtime in this process, bit mask.  The engine's three launches per simulation step are
 * ~6 % faster with kernel arguments in device memory (HIP_FORCE_DEV_KERNARG=1), which the HIP runtime reads ONCE, when
 * it initialises:
 *   bit 0  HIP_FORCE_DEV_KERNARG=1 is in the process environment
 *   bit 1  ... and it was put there by this library's load hook (the host had not set it): it is effective only if the
 *          host had not initialised HIP before loading libsc_engine.so -- which the library cannot observe.  Hosts that
 *          load torch/tch first should export the variable themselves; then bit 1 is clear.
 *   bit 2  the load hook was disabled by SC_ENGINE_KEEP_ENV=1 (the library never touches the environment)
 * sc_engine_create leaves a note in sc_last_warning() when bit 0 is clear or bit 1 is set. */
int sc_runtime_flags(void);
const char* sc_last_warning(void);

/* ------------------------------------------------------------------ network (L-predict) */
enum { SC_PREC_BF16 = 0, SC_PREC_FP8 = 1 };
typedef struct {
    int32_t n_res_blocks;  /* py/module.py:110 (reference default 19) */
    int32_t channels;      /* trunk width: 256 in the reference (py/module.py:120-133); 128 = BASELINE cfg2 variant */
    uint64_t seed;         /* used when weights_path == NULL: build-owned deterministic init (tools/scw.py) */
    int32_t precision;     /* SC_PREC_BF16: the reference's exported precision (py/export.py:47-65, bf16 autocast).
                              SC_PREC_FP8 (BASELINE configs[4]): the convs (stem, blocks, head convs) run on the CDNA4 fp8
                              matrix cores -- OCP e4m3 operands, per-output-channel power-of-two weight scales, fp32
                              accumulate; LayerNorm / residual stream / softmax fp32 and the SE + value FC layers bf16 as
                              before.  Stated tolerance vs the fp32 reference vectors: prior total
                              variation < 0.05, |value| error < 0.05 -- on init-scale outputs, where it is met.  On the
                              reference's vectors at a trained net's output range (policy gain x 4) the forward test measures
                              a prior total variation of 0.145 and asserts 0.25 (tests/test_gpu_parity2.py).  In the search
                              (sharp 6 x 128 networks, 48 positions, rollout 96, against the fp32 network's root visit
                              shares; tests/test_gpu_sharp_search.py): mean total variation 0.067
                              (gain x 4, value layer x 2) and 0.101 (gain x 8), the fp32 network's most visited move among
                              the engine's on 44 and 41 of 48; bf16: 0.005 and 0.006, 48 of 48. */
    int32_t reserved;
} sc_net_config;

/* Replaces backend construction in src/main.rs:83-128 (ChessTS / ChessEP / ChessOnnx).
 * weights_path: NULL, or a blob written by tools/scw.py / tools/ckpt_to_scw.py from a reference state_dict: SCW1 (fp32
 * tensors; quantised at load as cfg->precision asks) or SCW2 (the fp8 export: e4m3 conv weights + their channel scales;
 * the blob's precision wins).  An SCW2 channel may carry any exponent in [-100, 100]; it is kept as it is (E8M0 scale byte
 * 127 + e).  Contract: any lossless split of a channel -- every way to write its weights as e4m3 * 2^e -- gives the same
 * network: the same real weights, the same bits wherever the partial sums of a conv leave the fp32 accumulator bits to spare,
 * and elsewhere results that differ by the accumulator's last bits only (tests/test_gpu_fp8_splits.py). */
int sc_engine_create(const sc_net_config* cfg, const char* weights_path, int device_id, sc_engine** out);
void sc_engine_destroy(sc_engine*);
int sc_engine_max_batch(const sc_engine*);
int sc_engine_precision(const sc_engine*);   /* SC_PREC_* the engine runs in */

/* ChessModule.forward on a batch (src/backends/torch.rs:115-125, py/module.py:135-154):
 * host buffers in, logp [n][4672] fp32 (log-softmax, channel-major flatten) and value [n] out
 * (value from White's point of view).  logp may be NULL. */
int sc_forward_batch(sc_engine*, int n, const int8_t* boards, const int32_t* meta, float* logp, float* value);

/* The post-_encode tail of Game::predict (src/backends/torch.rs:108-146): forward, gather the
 * legal action logits, exp, renormalise by (sum + 1e-5) (src/chess.rs:891-901).
 * legal_idx / priors are CSR: position i owns [legal_off[i], legal_off[i+1]). */
int sc_predict_batch(sc_engine*, int n, const int8_t* boards, const int32_t* meta, const uint16_t* legal_idx,
                     const uint32_t* legal_off, float* priors, float* value);

/* Game::predict with argmax = true (the reference passes it from chess_play_inference, src/lib.rs:333-337): the same, then
 * post_process_distr's argmax branch (src/chess.rs:880-889) -- priors become a one-hot vector at the LAST maximum of each
 * position (Iterator::max_by). */
int sc_predict_batch_argmax(sc_engine*, int n, const int8_t* boards, const int32_t* meta, const uint16_t* legal_idx,
                            const uint32_t* legal_off, float* priors, float* value);
int sc_engine_synchronize(sc_engine*);
/* test aid: fp32 residual stream [n][64][channels] after `stage`: 0 = after conv_block, b = after the b-th residual block (1-based:
 * 1 is the first block), 1000 = trunk output */
int sc_forward_debug(sc_engine*, int n, const int8_t* boards, const int32_t* meta, int stage, float* out);

/* Rules + encoder on the GPU: replaces python-chess (src/chess.rs:665-803) and _encode
 * (src/chess.rs:845-877) for positions given as move lists from the start position (from any position:
 * sc_encode_positions_from).
 * For position i (moves[move_off[i]..move_off[i+1])):
 *   boards[i], meta[i]                      the NN input
 *   legal_moves[i][..], legal_idx[i][..]    legal moves in python-chess generation order and their
 *                                           action indices (row stride SC_MAX_MOVES), n_legal[i]
 *   outcome[i][0] = termination (src/chess.rs:88-99 numbering, 0 = none; outcome(claim_draw=True)),
 *   outcome[i][1] = winner (1 white, 0 black, -1 none), outcome[i][2] = is_check, outcome[i][3] = 0 ok / <0 illegal move at that index-1
 * Any output pointer may be NULL. */
int sc_encode_positions(sc_engine* engine_or_null, int device_id, int n, const uint16_t* moves, const uint32_t* move_off,
                        int8_t* boards, int32_t* meta, uint16_t* legal_moves, uint16_t* legal_idx, int32_t* n_legal,
                        int32_t* outcome);

/* Trace -> training tensors on the GPU: replaces libsmartchess.chess_encode_steps
 * (reference src/lib.rs:46-128; consumer py/dataset.py:47-87) for a batch of recorded games.
 *   moves / move_off     the played moves of game g: moves[move_off[g] .. move_off[g+1]); ply p (global index, game after
 *                        game) is the position BEFORE moves[p]
 *   child_mv / child_n / child_off   the searched children of ply p and their visit counts: [child_off[p], child_off[p+1])
 *                        (a trace's steps[i][2] = [[uci, N, Q, uct], ...]; at most SC_MAX_MOVES per ply)
 *   apply_mirror         the reference's colour-mirror augmentation (changes meta only; py/dataset.py negates the outcome)
 * Outputs, host pointers, any of the first five may be NULL (P = move_off[n_games] plies):
 *   boards int8[P][8][8][112], meta int32[P][7], dist float[P][4672] = N_i / (sum N + 1e-5) at the action index of
 *   the real mover, legal_idx uint16[P][SC_MAX_MOVES] + n_legal int32[P] (the reference's `move_indices`),
 *   status int32[n_games]: 0 ok; 1000+i: the children of ply i are not exactly the legal moves ("inconsistent moves",
 *   the reference panics, lib.rs:64-76); -(i+1): the move played at ply i is not legal (lib.rs:78-80).  Outputs of a
 *   game at and after its failing ply are unspecified. */
int sc_encode_steps(sc_engine* engine_or_null, int device_id, int n_games, const uint16_t* moves, const uint32_t* move_off,
                    const uint16_t* child_mv, const uint32_t* child_n, const uint32_t* child_off, int apply_mirror,
                    int8_t* boards, int32_t* meta, float* dist, uint16_t* legal_idx, int32_t* n_legal, int32_t* status);

/* measurement aid (bench.py also_encode_steps): the last sc_encode_steps call of the calling thread -- HIP-event time of the
 * encoder work it enqueues, summed over its slices (per slice: the upload of the slice's moves, children and offsets, the ply
 * index, game walk, keys, repetition flags, planes + moves, dist, status codes; not the copy-out) and wall time of the whole call
 * including the PCIe copies */
int sc_encode_steps_last_timing(float* kernels_ms, float* total_ms);

/* Training tensors straight into DEVICE memory, for a trainer on the same GPU (no copy through the host).
 * sc_encode_steps_device takes the host inputs of sc_encode_steps; sc_selfplay_encode_traces reads finished games from the
 * self-play handle's trace ring in place.  Outputs (P = plies of the call), device pointers, any may be NULL except status:
 *   layout 0 (reference): boards int8 [P][8][8][112], meta int32 [P][7] -- bit-identical to sc_encode_steps
 *   layout 1 (trainer, py/dataset.py _prepare): boards float32 [P][112][8][8] (channel-major), meta float32 [P][7]: the same
 *            integers, converted exactly
 *   dist float32 [P][4672] as sc_encode_steps; legal_idx uint16 [P][SC_MAX_MOVES] and n_legal int32 [P] as sc_encode_steps
 *   dist_legal float32 [P][SC_MAX_MOVES]: entry i = the visit share of legal move i (the same float dist holds at
 *            legal_idx[p][i]), 0 past n_legal.  The dense row is  zeros(P, 4672).scatter_add_(1, legal_idx.long(), dist_legal)
 *            -- scatter_add_, NOT scatter_: the padding entries point at action 0, which can be a legal move, and a plain
 *            scatter would overwrite its share with the padding's 0.
 *   status int32 [n_games] (device): sc_encode_steps's codes (0, 1000+i, -(i+1): the first failing ply of the game, a
 *            children mismatch before an illegal move at the same ply), reduced on the device.
 * Output pointers are checked (hipPointerGetAttributes): host memory or memory of another GPU than the engine's / handle's /
 * device_id's returns -1.
 * Stream contract: `stream` is a hipStream_t (NULL: the default stream).  The call returns once the work is enqueued on it and
 * does not synchronise; read the outputs after the stream's work (e.g. hipStreamSynchronize).  Its scratch memory is a
 * per-device arena the library keeps: an event recorded behind each call's work makes the next call (on any stream) wait for
 * it on the device, and only growing the arena waits on the host for the previous call before freeing the old buffer.  Keep
 * the host input arrays unchanged until the work is done (they are uploaded with hipMemcpyAsync on `stream`).
 * Returns 0, or < 0 as every entry point (-3: no HIP device). */
int sc_encode_steps_device(sc_engine* engine_or_null, int device_id, int n_games, const uint16_t* moves, const uint32_t* move_off,
                           const uint16_t* child_mv, const uint32_t* child_n, const uint32_t* child_off, int apply_mirror, int layout,
                           void* stream, void* boards, void* meta, float* dist, float* dist_legal, uint16_t* legal_idx,
                           int32_t* n_legal, int32_t* status);

/* ------------------------------------------------------------------ games written as SAN movetext (PGN, the reference's sample.csv) */
/* One game's movetext -> one token per half-move, on the host (no GPU is needed).  A token holds the SAN characters of the
 * half-move, character k in byte k of the uint64 (little-endian), zero-padded, at most 7 of them, with the suffix run of + # ! ?
 * stripped: "Nbd2", "exd8=Q", "O-O-O".  Skipped: move numbers ("12.", "12...", glued "1.e4"), {...} comments, ; comments to the
 * end of the line, (...) variations (nested; comments inside them are opaque), $n NAGs, [...] header tags, annotation glyphs
 * standing alone.  The text ends at a result token (1-0, 0-1, 1/2-1/2, *) or after `len` bytes; it need not be zero-terminated.
 * Anything else -- a word of more than 7 characters after stripping, a closing bracket that closes nothing -- is stored as the
 * reserved value 0xFFFFFFFFFFFFFFFF, which sc_encode_san_device reports as malformed at that ply: the token count stays the
 * number of half-moves of the text.
 * *n_tokens = that count.  If it exceeds cap the call returns SC_ERR_CAPACITY; the first cap tokens are written and nothing past
 * them (tokens may be NULL with cap 0: a count query). */
int sc_san_tokenize(const char* text, size_t len, uint64_t* tokens, uint32_t cap, uint32_t* n_tokens);

/* SAN tokens -> moves and training tensors in one call: the reference's ValidationDataset (py/dataset.py:90-128, python-chess's
 * read_game + parse_san, then chess_encode_steps on a trace whose children are the legal moves with count 1 on the move played
 * and 0 elsewhere) for a batch of games from the start position.
 *   tokens / tok_off   host, as moves / move_off of sc_encode_steps_device: the tokens of game g are tokens[tok_off[g] ..
 *                      tok_off[g+1]), P = tok_off[n_games]; at most 4000 per game
 * The parser runs on the device, one wavefront per game, against the generated legal moves.  Grammar: python-chess's SAN pattern
 * with upper-case pieces, [NBRQK]?[a-h]?[1-8]?[x-]?[a-h][1-8](=?[NBRQ])?, and O-O / O-O-O written with the letter O or the digit
 * 0.  A legal move answers to a token when its destination and promotion piece (none = none) are the token's, the moving piece
 * is the named one (a pawn when none is named) and its origin file and / or rank is what the token gives; castling is the king's
 * move from the e-file to the g- / c-file of the mover's back rank.  Over-specified disambiguation is accepted; the capture mark
 * is not verified (python-chess does not either).  Since only LEGAL moves are candidates, "Nd2" is unique when the other knight
 * is pinned.  Claimable draws do not end a game (read_game plays on too).
 * Outputs, device pointers, any may be NULL except status; pointer checks, layouts, stream contract and scratch arena as
 * sc_encode_steps_device; the parsed moves reach the encoder in device memory, nothing returns to the host in between.
 *   boards, meta, legal_idx, n_legal   as sc_encode_steps_device for the parsed moves
 *   dist, dist_legal   float32(1 / (1 + 1e-5)) at the move played, 0 elsewhere: bit-identical to sc_encode_steps_device given
 *                      those children
 *   moves   uint16 [P]: the parsed moves (a call with only moves and status is plain "SAN -> moves": no encoder work is enqueued)
 *   status  int32 [n_games]: 0 ok; -(i+1): token i names no legal move (any token after mate or stalemate does); 100000 + i:
 *           token i answers to more than one legal move; 200000 + i: token i is malformed or the reserved value.  The first
 *           failing ply of a game wins and the other games of the call are not affected; outputs of a game at and after its
 *           failing ply are unspecified.
 * Returns 0, or < 0 as every entry point (-3: no HIP device). */
int sc_encode_san_device(sc_engine* engine_or_null, int device_id, int n_games, const uint64_t* tokens, const uint32_t* tok_off,
                         int apply_mirror, int layout, void* stream, void* boards, void* meta, float* dist, float* dist_legal,
                         uint16_t* legal_idx, int32_t* n_legal, uint16_t* moves, int32_t* status);

/* ------------------------------------------------------------------ positions given as FEN / EPD: a base for every entry point */
/* FEN or EPD text -> the raw fields of a position, on the host (no GPU is needed, the rules code is not called).  Every read is
 * bounded by `len`; the text need not be zero-terminated.  Fields are separated by runs of white space.  Grammar: python-chess's
 * Board.set_fen for standard chess --
 *   1 board     eight ranks separated by '/', each of digits 1-8 and letters of pnbrqkPNBRQK that sum to 8, no two digits in a row
 *   2 turn      w | b
 *   3 castling  - | up to two of KQ, then up to two of kq, no letter twice (Shredder / X-FEN file letters: refused, no Chess960)
 *   4 ep        - | [a-h][36]
 *   5, 6 clocks present when the fifth AND the sixth word are integers (-?[0-9]+): halfmove 0..65535, fullmove 0..65535 with 0 read
 *               as 1.  Anything else behind the fourth field -- EPD operations such as "bm Qh5;" -- is ignored: halfmove 0, fullmove 1.
 * Returns 0, or -(number of the failing field, 1..6) with *out zeroed; a missing field fails as that field (an empty text: -1).
 * castling: bit 0 K, 1 Q, 2 k, 3 q as written (not yet checked against the board); ep: the square as written (a1 = 0) or -1;
 * occ[1] White's men, occ[0] Black's; pcs by piece type p n b r q k.  Whether the position can be played is decided on the device
 * (sc_positions_from_fen). */
struct sc_fen_fields {
    uint64_t pcs[6];
    uint64_t occ[2];
    int32_t turn;      /* 1 White, 0 Black */
    int32_t castling;
    int32_t ep;
    int32_t halfmove;
    int32_t fullmove;
    int32_t reserved;
};
typedef struct sc_fen_fields sc_fen_fields;
int sc_fen_parse(const char* text, size_t len, sc_fen_fields* out);

/* A set of n positions in device memory, validated there: the base of a move list wherever an entry point ends in _from.
 * fens[i]: zero-terminated FEN / EPD text, or NULL for the start position.  One wavefront per position writes its record in the
 * form the library keeps everywhere: castling rights cleaned (king and rook on their squares), the ep square kept only if
 * python-chess's _valid_ep_square holds (the right rank for the side to move, an enemy pawn in front of it, the square and the
 * one behind it empty; otherwise dropped, which is no error), the transposition key, no flags.  Status of position i:
 *      0  playable
 *      1  the game is already over here: no legal move, or outcome(claim_draw=True) is set (insufficient material, halfmove >= 100 ...)
 *     -1  not exactly one king per side
 *     -2  a pawn on rank 1 or 8
 *     -3  the side that is NOT to move is in check
 *     -4  material no game can reach: more than 16 men or 8 pawns of a colour, or more promoted pieces than missing pawns
 *     -5  more than two checkers
 *     -6  the fields contradict each other (a square with two pieces, or a piece without a colour): sc_fen_parse never writes such
 *   -(100 + f)  sc_fen_parse refused field f
 * The checks run in that order, before the move generator sees the position; the first failing one wins, the other positions of
 * the call are not affected, and the call still returns the set (0), so that a suite reader can report every bad line at once.
 * The record of a refused position is the start position's; no consumer reads it.  status (host, may be NULL) int32 [n].
 * Consumers refuse (-1, sc_last_error) an entry whose status is negative, and one whose status is 1 wherever a search would
 * start from it.  sc_positions_fen: python-chess's Board.fen() of entry i -- the ep square is printed only if a legal en-passant
 * capture exists, found on the device when the set was made -- returns the length, writes at most cap bytes with the final zero;
 * < 0 for an entry whose status is negative.  Returns < 0 as every entry point (-3: no HIP device). */
typedef struct sc_positions sc_positions;
int sc_positions_from_fen(int device_id, int n, const char* const* fens, sc_positions** out, int32_t* status);
void sc_positions_destroy(sc_positions*);
int sc_positions_count(const sc_positions*);
int sc_positions_status(const sc_positions*, int i);
int sc_positions_fen(const sc_positions*, int i, char* buf, int cap);

/* ------------------------------------------------------------------ perft on the device: node counts, divide, move kinds */
/* The legal move sequences of exactly `depth` moves from each of n entries, counted by the device rules (gen_legal_wave,
 * make_move): the number every move generator is compared by.  All pointers are host pointers; the call is synchronous.
 * Entry i is bases[base_idx[i]] followed by moves[move_off[i] .. move_off[i+1]), as sc_encode_positions_from reads them:
 * base_idx[i] < 0, or base_idx == NULL, or bases == NULL: the start position; moves == NULL with move_off == NULL: no entry has
 * moves.  A base whose status is negative refuses the call (-1, nothing is written); a base whose status is 1 is accepted.
 *   status[i]   0, or -(j+1): move j of the entry's list is not legal.  Such an entry has nodes 0, zero kinds and n_div 0; the
 *               other entries are not affected.
 *   nodes[i]    the number of sequences; depth 0: 1.  Only "no legal move" ends a line: repetitions, the fifty-move count and
 *               insufficient material do not, as in every published perft table.  depth: 0..16.
 *   kinds[i][k] over the LAST moves of those sequences (the Chess Programming Wiki's columns): SC_PERFT_CAPTURES (en passant
 *               included), _EP, _CASTLES, _PROMOTIONS, _CHECKS (the side to move after the last move is in check; mates are
 *               included), _CHECKMATES.  Slot SC_PERFT_NODES repeats nodes[i], slot 7 is written 0; depth 0: slots 1-7 are 0.
 *   divide      n_div[i]: the legal moves of entry i (0 at depth 0 and for a refused entry); div_moves[i][k]: those moves in the
 *               generator's order (python-chess's), not sorted; div_nodes[i][k]: the sequences that begin with move k.  Both rows
 *               are written 0 from n_div[i] on; the row of div_nodes sums to nodes[i].
 * max_frontier: the node records (72 bytes) a level buffer holds; 0: 2^20; otherwise 256..2^24.  A level that outgrows it is
 * walked in pieces; no output depends on it.  The call's device memory -- at most `depth` such buffers and 8 bytes per record of
 * counts and offsets, plus the outputs -- is allocated for the call and freed when it returns.
 * n: 0..2^24-1 (n == 0 is valid and touches nothing).  Integer sums only: identical calls give identical bytes.
 * Returns 0, or < 0 as every entry point (-3: no HIP device; argument errors are found before a device is looked for).
 * sc_perft_last_timing: measurement aid (tools/perft_rate.py) -- of the calling thread's last sc_perft, the HIP-event time of its
 * kernel launches, summed over the stretches between two host reads, and the wall time of the whole call. */
enum { SC_PERFT_NODES = 0, SC_PERFT_CAPTURES = 1, SC_PERFT_EP = 2, SC_PERFT_CASTLES = 3,
       SC_PERFT_PROMOTIONS = 4, SC_PERFT_CHECKS = 5, SC_PERFT_CHECKMATES = 6 /* 7: reserved, written 0 */ };
int sc_perft(int device_id, int n, const sc_positions* bases, const int32_t* base_idx,
             const uint16_t* moves, const uint32_t* move_off, int depth, int max_frontier,
             uint64_t* nodes      /* [n]            required   */,
             uint64_t* kinds      /* [n][8]         or NULL    */,
             uint16_t* div_moves  /* [n][224]       or NULL    */,
             uint64_t* div_nodes  /* [n][224]       or NULL; NULL exactly when div_moves is */,
             int32_t*  n_div      /* [n]            or NULL    */,
             int32_t*  status     /* [n]            or NULL    */);
int sc_perft_last_timing(float* kernels_ms, float* total_ms);

/* sc_encode_positions with a base per position: position i is bases[base_idx[i]] followed by its moves; base_idx[i] < 0, or
 * base_idx == NULL, or bases == NULL: the start position, and the outputs are those of sc_encode_positions.  History planes
 * older than the base are zero; repetitions and the fifty-move count start at the base (its halfmove clock counts).  A base whose
 * status is 1 is encoded like any other (its outcome says why the game is over). */
int sc_encode_positions_from(sc_engine* engine_or_null, int device_id, int n, const sc_positions* bases, const int32_t* base_idx,
                             const uint16_t* moves, const uint32_t* move_off, int8_t* boards, int32_t* meta, uint16_t* legal_moves,
                             uint16_t* legal_idx, int32_t* n_legal, int32_t* outcome);
/* sc_encode_steps_device / sc_encode_san_device with a base per game (base_idx host int32 [n_games], as above): the plies of game g
 * start at its base.  The set must live on the call's device and stay alive until the stream's work is done. */
int sc_encode_steps_device_from(sc_engine* engine_or_null, int device_id, int n_games, const sc_positions* bases, const int32_t* base_idx,
                                const uint16_t* moves, const uint32_t* move_off, const uint16_t* child_mv, const uint32_t* child_n,
                                const uint32_t* child_off, int apply_mirror, int layout, void* stream, void* boards, void* meta,
                                float* dist, float* dist_legal, uint16_t* legal_idx, int32_t* n_legal, int32_t* status);
int sc_encode_san_device_from(sc_engine* engine_or_null, int device_id, int n_games, const sc_positions* bases, const int32_t* base_idx,
                              const uint64_t* tokens, const uint32_t* tok_off, int apply_mirror, int layout, void* stream, void* boards,
                              void* meta, float* dist, float* dist_legal, uint16_t* legal_idx, int32_t* n_legal, uint16_t* moves,
                              int32_t* status);

/* ------------------------------------------------------------------ moves written as SAN movetext and PGN */
/* Moves -> SAN tokens on the device, the inverse of sc_encode_san_device: python-chess's Board.san() for every ply of a batch of
 * games.  moves / move_off: host, as sc_encode_steps_device takes them (at most 4000 plies per game); tokens uint64 [P] and
 * status int32 [n_games] are device pointers, both required; pointer checks, stream contract and scratch arena as
 * sc_encode_steps_device.  One wavefront per ply renders its move against the generated legal moves of the position before it
 * and takes the check mark from those of the position after it.
 *   tokens[p]  sc_san_tokenize's format (character k in byte k, zero-padded) WITH the suffix: "Nbd2", "exd8=Q#", "O-O-O+", at most
 *              7 characters.  Disambiguation is python-chess's: among the other LEGAL moves of a piece of the same kind to the same
 *              square -- none: nothing; one on the origin's rank: the file letter; one on the origin's file: the rank digit;
 *              neither: the file letter.  Pawns: the origin file when they capture (en passant included).  '+' check, '#' mate,
 *              stalemate has no mark.
 *   status[g]  0, or -(i+1): move i of the game is not legal there (the first such ply).  The game's tokens from ply i on are 0;
 *              the other games of the call are not affected.
 * n_games == 0 and games without plies are valid; nothing is written beyond tokens[P) and status[n_games).
 * _from: a base per game as sc_encode_steps_device_from.  Returns 0, or < 0 as every entry point (-3: no HIP device). */
int sc_moves_to_san_device(int device_id, int n_games, const uint16_t* moves, const uint32_t* move_off, void* stream, uint64_t* tokens,
                           int32_t* status);
int sc_moves_to_san_device_from(int device_id, int n_games, const sc_positions* bases, const int32_t* base_idx, const uint16_t* moves,
                                const uint32_t* move_off, void* stream, uint64_t* tokens, int32_t* status);
/* Tokens -> one line of movetext, on the host (no GPU is needed): "1. e4 e5 2. Nf3" from move number `fullmove`, or with
 * black_first "12... Nf6 13. d4"; `result` (may be NULL) is appended as the last word; a token of 0 ends the moves.  Returns the
 * length of the whole text and writes at most cap bytes with the final zero, like sc_positions_fen (cap 0: a length query, buf may
 * be NULL); < 0: bad argument. */
int sc_san_format(const uint64_t* tokens, uint32_t n, int fullmove, int black_first, const char* result, char* buf, size_t cap);

/* ------------------------------------------------------------------ trace files read on the device */
/* The text of n trace files (sc_trace_write_json / sc_selfplay_write_trace_json, the reference's Trace::save) -> the played moves,
 * the children with their visit counts, the outcome and the optional "opening" / "fen" members, parsed by kernels and kept in
 * device memory behind a handle, where sc_traces_encode_device reads them: no move or child comes back to the host on the way to
 * the training tensors.
 *
 * This reads MACHINE-WRITTEN traces.  It is NOT a JSON validator: it refuses what the table below lists and may accept or refuse
 * other text a strict parser would refuse ("[1 2]", "[ }"); such text never disturbs the other files of the call and never makes
 * a count exceed the limits.
 *   characters   the top level is one object; white space is space, \t, \n, \r; strings hold no backslash (no string the writers
 *                produce needs one) and may hold bytes >= 0x80; true / false appear nowhere.
 *   members      at depth 1, in any order and with any white space (the pretty form of the writer, json.dumps with any indent or
 *                with separators=(",", ":"), CRLF line ends).  "steps": exactly once, an array (may be empty) of steps
 *                [move string, one number or null, [children]]; a child is an array [move string, unsigned decimal integer <=
 *                4294967295, ...]: what follows the count (Q, uct) is skipped and NOT parsed -- no float leaves this reader.
 *                A move string is [a-h][1-8][a-h][1-8][nbrq]?.  "outcome": null, or an object of "winner" ("White", "Black" or null)
 *                and "termination" (a name of the writer's table); absent: has_outcome 0.  "opening": an array of move strings.
 *                "fen": a string of at most 127 bytes.  Any other member is ignored, whatever it holds.
 *   limits       at most 4000 steps, at most SC_MAX_MOVES children per step; runs of up to 255 white-space bytes between tokens
 *                are accepted, a longer run is read or refused with SC_TRACE_ERR_SPACE.
 * A refused file has status -code, counts 0 and no entry in the packed arrays; the call still returns 0 and the set, the other
 * files are not affected.  err_at: the byte offset in the file of the first defect -- the smallest offset wins, at one offset the
 * smaller code; what is only known at the end of the text (an open string, open brackets, no "steps") counts at the file's length.
 *   SC_TRACE_ERR_UNBALANCED  the text ends inside a string or with open brackets; a closing bracket closes nothing; the first
 *                            token is not '{'; the file is empty
 *   SC_TRACE_ERR_ESCAPE      a backslash inside a string (err_at: the backslash)
 *   SC_TRACE_ERR_STEPS       no "steps" array at depth 1, or more than one
 *   SC_TRACE_ERR_SHAPE       a step or a child is not an array that starts with a string; a step holds no children array or more
 *                            than one; a child's second element is missing
 *   SC_TRACE_ERR_MOVE        a move string (step, child or opening) is not UCI as above (err_at: its opening quote)
 *   SC_TRACE_ERR_COUNT       a child's second element is not an unsigned integer in range: sign, fraction, exponent, null,
 *                            overflow (err_at: the first byte of the token)
 *   SC_TRACE_ERR_CHILDREN    a step has more than SC_MAX_MOVES children
 *   SC_TRACE_ERR_PLIES       more than 4000 steps
 *   SC_TRACE_ERR_OUTCOME     "outcome" is of another form
 *   SC_TRACE_ERR_SPACE       more than 255 white-space bytes between two tokens where the reader had to step over them
 *
 * sc_traces_read: text holds the bytes of the n files one after another (host); file g is text[text_off[g] .. text_off[g+1]),
 * text_off[n] < 2^32.  Synchronous: the host sizes the handle's arrays from the parsed totals, and the uploaded text is freed
 * before the call returns.  n == 0 gives an empty set.  A non-monotonic text_off, or text_off[n] >= 2^32: -1 (found before a
 * device is looked for).
 * sc_traces_summary: per file, host arrays, any may be NULL: status int32 [n], err_at uint32 [n], n_steps / n_children / n_opening
 * uint32 [n], outcome int32 [n][3] = has_outcome, termination, winner (sc_trace_info's conventions), has_fen int32 [n].
 * sc_traces_get: host copies of games [g0, g0 + n), offsets rebased to 0, any may be NULL (sizes from sc_traces_summary):
 * move_off [n+1], moves, child_off [plies + 1], child_mv, child_n, open_off [n+1], opening.  Moves are the library's uint16
 * (from | to << 6 | promo << 12, n = 2 b = 3 r = 4 q = 5).
 * sc_traces_fen: the "fen" member of file g: its length, or 0 without one; writes as sc_positions_fen.
 * sc_traces_encode_device: games [g0, g0 + n) -> training tensors; outputs, layouts, pointer checks, stream contract and arena of
 * sc_encode_steps_device, on the handle's device (or the engine's, which must be the same).  Row p of the outputs is ply
 * p - move_off[g0] of the range.  The moves are copied on the device, the children are read in place; the handle must stay alive
 * until the stream's work is done.  status[g] (device, required): 0; 1000 + i and -(i + 1) as sc_encode_steps_device;
 * 300000 + code: the reader refused the file with that code (the game has no plies); 400000: the file has an "opening" or a
 * "fen" member, so its steps do not start at the start position (such a game keeps its rows, whose contents are unspecified).
 * sc_traces_last_timing: measurement aid (tools/trace_read_rate.py) -- HIP-event time of the two parse passes of the calling
 * thread's last sc_traces_read (the counting pass with the scans of its counts, the emitting pass).
 * Returns 0, or < 0 as every entry point (-3: no HIP device). */
#define SC_TRACE_ERR_UNBALANCED 1
#define SC_TRACE_ERR_ESCAPE 2
#define SC_TRACE_ERR_STEPS 3
#define SC_TRACE_ERR_SHAPE 4
#define SC_TRACE_ERR_MOVE 5
#define SC_TRACE_ERR_COUNT 6
#define SC_TRACE_ERR_CHILDREN 7
#define SC_TRACE_ERR_PLIES 8
#define SC_TRACE_ERR_OUTCOME 9
#define SC_TRACE_ERR_SPACE 10
typedef struct sc_traces sc_traces;
int sc_traces_read(int device_id, int n, const char* text, const uint64_t* text_off, sc_traces** out);
void sc_traces_destroy(sc_traces*);
int sc_traces_count(const sc_traces*);
int sc_traces_summary(const sc_traces*, int32_t* status, uint32_t* err_at, uint32_t* n_steps, uint32_t* n_children,
                      uint32_t* n_opening, int32_t* outcome, int32_t* has_fen);
int sc_traces_get(const sc_traces*, int g0, int n, uint32_t* move_off, uint16_t* moves, uint32_t* child_off,
                  uint16_t* child_mv, uint32_t* child_n, uint32_t* open_off, uint16_t* opening);
int sc_traces_fen(const sc_traces*, int g, char* buf, int cap);
int sc_traces_encode_device(sc_engine* engine_or_null, const sc_traces*, int g0, int n, int apply_mirror, int layout, void* stream,
                            void* boards, void* meta, float* dist, float* dist_legal, uint16_t* legal_idx, int32_t* n_legal,
                            int32_t* status);
int sc_traces_last_timing(float* count_ms, float* emit_ms);

/* ------------------------------------------------------------------ network on device tensors: forward, losses, agreement */
/* sc_forward_batch on DEVICE pointers: boards int8 [n][8][8][112] and meta int32 [n][7] as layout 0 of sc_encode_steps_device
 * leaves them, logp float [n][4672] (may be NULL) and value float [n] in device memory of the engine's GPU.  The same kernels as
 * sc_forward_batch: the outputs are bit-identical to it.  Every pointer is checked (hipPointerGetAttributes): host memory or
 * memory of another GPU returns -1.
 * Stream contract: `stream` is a hipStream_t (NULL: the default stream).  The call returns once the work is enqueued on it,
 * ordered after the earlier work of `stream` and of the engine, and does not synchronise; read the outputs after the stream's
 * work.  Only growing the engine's scratch (value-head features and split-K partials of up to 8 192 positions: longer inputs are
 * processed in slices of that many) waits on the host, for the engine's earlier work.  Later calls on the engine wait on the device
 * for this one.  As everywhere, one host thread drives an engine at a time. */
int sc_forward_device(sc_engine*, int n, const int8_t* boards, const int32_t* meta, void* stream, float* logp, float* value);

/* A network judged on recorded search results (the reference's scripts/train.py validation_step: compute_loss1, compute_loss2,
 * and training_step's pi_entropy), on the tensors one sc_encode_steps_device / sc_selfplay_encode_traces call with layout 0
 * leaves in device memory.  Inputs, device pointers (P = n positions): boards, meta as sc_forward_device; the visit shares in
 * exactly ONE of two forms -- dist float [P][4672] (16-byte aligned), or dist_legal float [P][SC_MAX_MOVES] + legal_idx uint16
 * [P][SC_MAX_MOVES] + n_legal int32 [P], of which only entries i < n_legal[p] are read (the padding points at action 0 with share
 * 0; 0 * logp is never formed); outcome float [P]: White's result of the position's game.  The other form's pointers are NULL;
 * both forms, or neither, return -1.
 * Outputs, device pointers, each may be NULL, float [P]:
 *   ce[p]    = -sum dist * logp over the entries with a non-zero share   (compute_loss1 before the division by the batch size)
 *   se[p]    = (value[p] - outcome[p])^2                                 (compute_loss2 before the mean; both White-relative)
 *   ent[p]   = -sum_a exp(logp[a]) * logp[a] over all 4672 actions       (pi_entropy before the mean)
 *   value[p] = the network's value
 *   summary  double [5]: [0] P, [1] mean ce (= loss1), [2] mean se (= loss2), [3] mean ent (= pi_entropy), [4] the number of
 *            positions whose ce, se or ent is not finite.  Those positions are counted and left in: the means are then
 *            non-finite too, as torch's would be.  P = 0: five zeros.
 * n_legal[p] outside 0..218, or an action index >= 4672 among a position's legal moves, is found on the DEVICE (the call does not
 * read device memory on the host): nothing is read through it, ce[p] is NaN and the position is counted in summary[4].
 * Every sum over a row is a fixed tree 13 additions deep (score_kernels.hip); exp is expf.  A position's results depend on its
 * own rows only, not on P or on its place among the positions; the summary is reduced in double precision in a fixed order, without
 * atomics: identical calls give identical bits.
 * Pointer checks and stream contract as sc_forward_device; the scratch adds the log-probability rows of one slice of 8 192
 * positions (153 MB) and, for per-position outputs passed as NULL, 12 bytes per position. */
int sc_score_positions(sc_engine*, int n, const int8_t* boards, const int32_t* meta, const float* dist, const float* dist_legal,
                       const uint16_t* legal_idx, const int32_t* n_legal, const float* outcome, void* stream, float* ce, float* se,
                       float* ent, float* value, double* summary);

/* Agreement of two networks on the same positions (the reference's scripts/validate_model.py), any pairing of precisions, depths
 * and widths; both engines on the GPU that holds boards / meta (engines on two devices: -1).  Outputs, device pointers, each may
 * be NULL:
 *   tv[p] = 1/2 sum_a |exp(logp_a[p][a]) - exp(logp_b[p][a])|     dv[p] = |value_a[p] - value_b[p]|
 *   summary double [9]: [0] P, then mean, population standard deviation (numpy's default), max, min of tv: [1..4], and of dv:
 *   [5..8] (a NaN among the values makes the four figures NaN).  P = 0: nine zeros.
 * The same engine twice runs one forward pass and compares its rows with themselves.  Arithmetic, pointer checks and stream
 * contract as sc_score_positions; both engines' later work waits on the device for the call. */
int sc_compare_engines(sc_engine* a, sc_engine* b, int n, const int8_t* boards, const int32_t* meta, void* stream, float* tv,
                       float* dv, double* summary);

/* ------------------------------------------------------------------ training minibatches from the compact tensors */
/* The per-sample work of the reference's DataLoader over ChessDataset (py/dataset.py _prepare; scripts/train.py:331-353), for
 * positions already in device memory: sample b of the batch is built from row r = rows[b] of the tensors ONE
 * sc_encode_steps_device / sc_selfplay_encode_traces call with layout 0 leaves behind (boards int8 [n_src][8][8][112], meta int32
 * [n_src][7], dist_legal float [n_src][SC_MAX_MOVES], legal_idx uint16 [n_src][SC_MAX_MOVES], n_legal int32 [n_src]) plus outcome
 * float [n_src] -- 8 548 B per ply instead of the trainer layout's 47 392.  rows int32 [n_batch] (a row may repeat); mirror uint8
 * [n_batch] or NULL (none).  All array arguments are device pointers; boards, dist_legal, legal_idx, out_boards and out_dist
 * 16-byte aligned.  Outputs, each may be NULL:
 *   out_boards[b]  float [112][8][8] = (float) boards[r][square][plane]: signed, exact
 *   out_meta[b]    float [7] = meta[r], exact; with mirror[b] != 0 Board::rotate()'s meta as apply_mirror forms it: with
 *                  t = m[0], [1 - t, m[1] + (t == 1), m[4], m[5], m[2], m[3], m[6]].  Planes and dist do not change under the mirror
 *   out_dist[b]    float [4672]: zeros, and dist_legal[r][i] at legal_idx[r][i] for i < n_legal[r] ONLY (the padding points at
 *                  action 0, which can be a legal move) -- bit-identical to the dense dist the encoder writes for that ply
 *   out_outcome[b] float = outcome[r], negated with mirror[b] != 0 (py/dataset.py:61-62)
 *   n_bad          int32 [1], zeroed on the stream first: the number of samples with bad input, found on the DEVICE (the call
 *                  does not read device memory on the host).  rows[b] outside [0, n_src): nothing is read through it, all four
 *                  outputs of b are NaN.  n_legal[r] outside 0..218, or an action index >= 4672 among the first n_legal[r]:
 *                  nothing is written through it, out_dist[b] is all NaN, the other three outputs are as normal.
 * One kernel launch, one workgroup per sample (batch_kernels.hip); no global address is written twice: identical calls give
 * identical bits.  Pointer checks as sc_forward_device (host memory or memory of another GPU than device_id's: -1); negative
 * sizes: -1; n_batch == 0: nothing is enqueued or written.
 * Stream contract: the work is enqueued on `stream` (NULL: the default stream); the call does not synchronise, has no scratch and
 * keeps nothing after it returns.  Returns 0, or < 0 as every entry point (-3: no HIP device). */
int sc_gather_batch(int device_id, int n_src, int n_batch, const int32_t* rows, const uint8_t* mirror, const int8_t* boards,
                    const int32_t* meta, const float* dist_legal, const uint16_t* legal_idx, const int32_t* n_legal,
                    const float* outcome, void* stream, float* out_boards, float* out_meta, float* out_dist, float* out_outcome,
                    int32_t* n_bad);

/* ------------------------------------------------------------------ identical training positions merged, targets averaged */
/* Self-play in lockstep from one start position, or from opening lines used twice, writes the same network input many times with
 * contradicting targets.  This call groups rows of the compact tensors (the form sc_gather_batch reads) that are the same sample
 * input and writes one row per group: the input of the group's head, the mean visit shares, the mean outcome, and a count.  The
 * outputs have the form of the inputs, so sc_gather_batch and sc_score_positions read them as they are.
 * Positions and rows: position p (0 <= p < n_in) stands for source row r(p) = rows ? rows[p] : p (rows: device int32 [n_in]; NULL
 * needs n_in <= n_src); a source row may stand at several positions.  r(p) outside [0, n_src): nothing is read through it,
 * group_of[p] = -1, p belongs to no group and adds 1 to counts[1].
 * Same sample: positions a and b are the same sample iff the 7 168 board bytes are equal, the 28 meta bytes are equal, n_legal is
 * equal and lies in 0..218, and legal_idx[:n_legal] is equal entry by entry.  Padding past n_legal (garbage, NaN, indices up to
 * 65535) is never looked at.  A position whose n_legal is outside 0..218 is the same as nothing: a group of one whose row is
 * copied verbatim, and 1 more in counts[1].
 * Groups: the head of a group is its smallest position; groups are numbered by ascending head.  group_of[p] (int32 [n_in]) is the
 * group's number, out_first[j] the head's position, out_count[j] the group's size m.
 * The merged row j: out_boards, out_meta, out_n_legal and the whole 224-entry out_legal_idx row are the head's bytes;
 * out_dist_legal[j][i] for i >= n_legal is the head's bits; for i < n_legal it is s / (float)m, an IEEE division, with s = x_1,
 * s = s + x_k for k = 2..m over the members in ascending position, in float32; out_outcome[j] is formed in the same way.  For m = 1
 * the row is bit-identical to its source row.  Rows >= counts[0] of the outputs are not written.  Each output may be NULL.
 * counts (device int32 [4], zeroed on the stream first): [0] the number of groups, [1] bad positions (as above), [2] positions
 * whose bytes differed from the head of their key (see below), [3] the largest m.
 * Keys are a shortcut, never the decision: rows are found through a key of key_bits bits (128 in normal use; 0..128 accepted)
 * over exactly the bytes named above, and EVERY position is then compared byte for byte with the head its key points to.  A
 * position that differs becomes a group of its own, is never merged with anything and adds 1 to counts[2].  So unequal rows are
 * never merged, whatever the key; equal rows can fail to merge only behind a key clash, which at 128 bits does not happen, and
 * which is reported.  Values of key_bits below 128 exist so that this path can be tested.
 * Workspace: device memory of at least the bytes sc_merge_positions_workspace(n_in) reports (about 120 per position; no device is
 * needed to ask), used during the call's work on the stream only.  A smaller one: -1.
 * Determinism: no float atomic is used anywhere, the order of every sum is fixed by position: identical calls give identical bits.
 * Pointer checks as sc_forward_device, the workspace included (host memory or memory of another GPU than device_id's: -1);
 * boards, legal_idx, out_boards and out_legal_idx 16-byte aligned; negative sizes, n_in above 2^30 or key_bits outside 0..128: -1;
 * n_in == 0: four zeros go to counts and nothing else is written.
 * Stream contract as sc_gather_batch: the work is enqueued on `stream` (NULL: the default stream); the call does not wait on the
 * host and keeps nothing after it returns.  Returns 0, or < 0 as every entry point (-3: no HIP device). */
int sc_merge_positions_workspace(int n_in, size_t* bytes);
int sc_merge_positions(int device_id, int n_src, int n_in, const int32_t* rows /* or NULL: position p is row p, n_in <= n_src */,
                       const int8_t* boards, const int32_t* meta, const float* dist_legal, const uint16_t* legal_idx,
                       const int32_t* n_legal, const float* outcome, int key_bits, void* workspace, size_t workspace_bytes,
                       void* stream, int8_t* out_boards, int32_t* out_meta, float* out_dist_legal, uint16_t* out_legal_idx,
                       int32_t* out_n_legal, float* out_outcome, int32_t* out_count, int32_t* out_first, int32_t* group_of,
                       int32_t* counts /* [4] */);

/* ------------------------------------------------------------------ self-play (L-search) */
/* SYNTH: integer-hash evaluator for exact search-parity tests; SYNTH_COARSE: the same with 2-bit priors and values from
 * {-0.5, 0, 0.5} (exact PUCT ties between some siblings); SYNTH_UNIFORM: uniform priors, value 0 (every unvisited sibling
 * ties: find_max's last-maximum rule, src/mcts.rs:78-88, decides every descent) */
enum { SC_EVAL_NET = 0, SC_EVAL_SYNTH = 1, SC_EVAL_SYNTH_COARSE = 2, SC_EVAL_SYNTH_UNIFORM = 3 };

typedef struct {
    int32_t n_slots;            /* concurrent games on this GPU (BASELINE cfg2: 256) */
    int32_t n_games;            /* total games to play on this handle (slots are recycled) */
    int32_t rollout_num;        /* --rollout-num      src/main.rs:32-33,175-180 */
    int32_t num_steps;          /* -n/--num-steps     src/main.rs:35-36 */
    float cpuct;                /* --cpuct            src/main.rs:50-51 */
    float temperature;          /* --temperature      src/main.rs:47-48 */
    int32_t temperature_switch; /* --temperature-switch src/main.rs:53-54 */
    float epsilon;              /* --epsilon          src/main.rs:56-57 */
    int32_t with_noise;         /* 1 in selfplay (src/main.rs:195), 0 for NNPlayer::bestmove (src/play.rs:250) */
    int32_t outcome_gate;       /* outcome() is consulted only when ply index > gate (src/main.rs:223: 100) */
    int32_t evaluator;          /* SC_EVAL_NET / SC_EVAL_SYNTH */
    int32_t external_noise;     /* tests: root noise is taken from sc_selfplay_set_noise instead of the device RNG */
    uint64_t seed;
    uint64_t first_game_id;     /* global id of this handle's first game (sharding across GPUs/ranks) */
    int32_t trace_capacity;     /* traces kept on the device: 0 = n_games (every trace retrievable); >0 = ring of that
                                   many games (>= 2*n_slots): game k uses row k % capacity.  A row is never taken while
                                   its previous game is still being played (the new game waits); a FINISHED trace is
                                   overwritten (throughput runs) unless trace_hold is set */
    int32_t own_stream;         /* 1: this handle launches on its own HIP stream, so several handles (groups of games)
                                   of one engine overlap on the GPU: one group's tree work hides under another's network */
    int32_t tie_random;         /* temperature 0: 0 = first most-visited child (mcts::step, src/mcts.rs:298-306);
                                   1 = uniformly random among the most visited (NNPlayer::bestmove, src/play.rs:268-277) */
    int32_t trace_hold;         /* 1: a finished trace stays in the ring until sc_selfplay_poll has handed it to the host and
                                   the host has polled again; new games wait for a free row (streaming drain: the reference
                                   writes each trace file when its game ends, src/main.rs:235-238) */
    float rollout_factor;       /* > 0: -r/--rollout-factor (src/main.rs:29-30,175-176): every ply searches
                                   min(300, (n_legal * factor) as i32) simulations, n_legal = legal moves of the ply's root;
                                   rollout_num must then be 300 (it sizes the node pools) */
} sc_selfplay_config;

int sc_selfplay_create(sc_engine* engine_or_null, int device_id, const sc_selfplay_config* cfg, sc_selfplay** out);
void sc_selfplay_destroy(sc_selfplay*);

/* Enqueue `n` simulation steps (each = one iteration of src/mcts.rs:261-288 for every active
 * game, including the per-ply move choice of mcts::step when a game's rollout count is reached). */
int sc_selfplay_enqueue_sims(sc_selfplay*, int n);
int sc_selfplay_synchronize(sc_selfplay*);
/* Enqueue n simulation steps on several handles of one GPU, interleaved step by step (handles created with
 * own_stream = 1 overlap on the device). */
int sc_selfplay_enqueue_interleaved(sc_selfplay** handles, int n_handles, int n);
/* Run until every game has finished (or max_sim_steps > 0 is reached). */
int sc_selfplay_run(sc_selfplay*, int64_t max_sim_steps);

typedef struct {
    int64_t sims_done;       /* simulations completed, all games */
    int64_t nn_evals;        /* leaf evaluations that needed the network */
    int32_t games_finished;
    int32_t games_active;
    int32_t error_flags;     /* bit mask: 1 non-finite PUCT value (reference panics: src/mcts.rs:202-214), 2 node pool overflow,
                                4 move without action index, 8 descent deeper than the path buffer, 16 / 32 internal hand-off timeout (search helper / value-head tiles) */
    int32_t plies_done;      /* total plies played over all games */
} sc_selfplay_stats;
int sc_selfplay_get_stats(sc_selfplay*, sc_selfplay_stats* out);
/* HIP-event timing on the stream the kernels are launched on.
 * enable_timing(stride > 0): every stride-th simulation step runs as three separate launches with the network TOWER launch
 *   bracketed by an event pair (the tower-only figure).
 * enable_timing(stride < 0): every |stride|-th simulation step is bracketed AS A WHOLE by an event pair, in whatever launch form
 *   the handle uses (one k_step launch in the production form): the duration of the dominant kernel as production runs it.
 * enable_timing(0): off.
 * timing(): ms_total = first enqueue -> last enqueue span; ms_nn = sum over the nn_launches sampled brackets (at most the last
 * 4096). */
int sc_selfplay_enable_timing(sc_selfplay*, int stride);
/* Match play (the `play` binary's loop, src/play.rs:318-343; batched: every slot is one game of the same pairing).
 * After this call the handle alternates players by ply: even plies are searched with `white`, odd plies with `black`
 * (engines for SC_EVAL_NET; for SC_EVAL_SYNTH the two salts select two deterministic synthetic players).
 * Needs n_games == n_slots (all games advance in lockstep, no slot recycling) and must precede the first enqueue.
 * Reference settings: with_noise = 0, outcome_gate = -1 (outcome after every ply), num_steps = 200, tie_random = 1. */
int sc_selfplay_set_players(sc_selfplay*, sc_engine* white, sc_engine* black, uint64_t synth_salt_white, uint64_t synth_salt_black);
/* Match play with slot recycling: n_games games on n_slots slots (any n_games >= 1), both colour assignments in one handle.
 * Players: a = index 0, b = index 1 (engines for SC_EVAL_NET, the two salts for the synthetic evaluators).  Simulation step t is
 * evaluated by player (t / rollout_num) & 1 for every slot, as with sc_selfplay_set_players; a game starts only at a ply
 * boundary (t % rollout_num == 0) whose step its White evaluates, so games of different ages share the handle and a finished
 * game's slot goes on with the next game.
 * Colour rule: colours = 0: a is White in every game.  colours = 1: the White of game k (0-based on this handle, k = game_id -
 * first_game_id) is player k & 1 -- a in the even games, b in the odd ones; with an odd n_games the extra game has a as White.
 * Every game 0..n_games-1 is played exactly once; game k is the game a lockstep handle of its pairing plays under the same
 * seed and game id.
 * Idle bound: a slot whose game ends takes a game that can start at once if one is left (its White evaluates the ply that
 * begins), else one of the other colour assignment, which starts one ply later: while games remain, a slot waits for at most
 * one ply between two games (with a trace ring, a game also waits for its row as on every handle; with colours = 1 an odd ring
 * size is used as the even number below it).  With colours = 0 a slot whose game ends after an odd number of plies waits one.
 * Preconditions as sc_selfplay_set_players without n_games == n_slots: before the first enqueue, rollout_factor = 0, both
 * engines on the handle's device and of the handle's split-K.  Reference settings as there.  < 0 on error (-3: no HIP device). */
int sc_selfplay_set_match(sc_selfplay*, sc_engine* a, sc_engine* b, uint64_t synth_salt_a, uint64_t synth_salt_b, int colours);
/* out[w*4 + r]: games finished so far with player w (0 = a, 1 = b) as White and
 * result r = 0 White won, 1 Black won, 2 draw, 3 no outcome.
 * Completes the enqueued work first.  Counted on the device when a game ends: it does not need the traces, which a ring
 * (trace_capacity > 0) overwrites.  -1 on a handle without sc_selfplay_set_match. */
int sc_selfplay_match_tally(sc_selfplay*, int64_t out[8]);
/* Opening lines for a match handle (after sc_selfplay_set_match, before the first enqueue; host pointers).
 * Line i = moves[move_off[i] .. move_off[i+1]) from the start position, 0..600 plies (an empty line is the start position).
 * Game ordinal k plays line (colours ? k >> 1 : k) % n_lines: with alternating colours games 2j and 2j+1 share a line.
 * status (may be NULL) int32 [n_lines]: 0 ok; -(j+1): move j of the line is not legal; 1: the line's last position
 * ends the game (outcome(claim_draw=True) is set, or there is no legal move).  Any non-zero status: returns -1 and the
 * handle is as before the call.
 * A game with a line of length L: its position chain 0..L (keys, repetition and irreversibility flags) is what
 * sc_selfplay_set_position leaves for that move list; the search starts at ply L, and the trace holds the searched plies only
 * (sc_selfplay_get_trace is unchanged).  num_steps, temperature_switch and outcome_gate count from the first searched ply; the
 * end-of-ply draw stays keyed by the absolute ply: the game is the CONTINUATION of the from-the-start game of the same id and
 * seed whose first L moves were the line.
 * Start rule: the first searched ply belongs to player white(k) ^ (L & 1), and the game starts at a ply boundary of that player;
 * a slot that draws a game of the other parity holds it for one ply, so the idle bound of sc_selfplay_set_match stands: at most
 * one ply between two games while games remain, apart from trace-ring waits.  The tally stays by White's player.
 * The lines are replayed and checked once, by this call; a game start copies L + 1 records on the device.
 * sc_selfplay_encode_traces refuses (-1) a game whose line is not empty: training tensors need the plies from the start. */
int sc_selfplay_set_openings(sc_selfplay*, int n_lines, const uint16_t* moves, const uint32_t* move_off, int32_t* status);
/* the line of handle-local game `game` (pure function of the table and the rule above): returns its length, writes up to cap moves */
int sc_selfplay_get_opening(sc_selfplay*, int game, uint16_t* moves, int cap);
/* Opening lines that start from bases: line i is entry base_idx[i] of `bases` (base_idx[i] < 0: the start position) followed by
 * its 0..600 moves; base_idx host int32 [n_lines].  bases == NULL or base_idx == NULL: sc_selfplay_set_openings.  Whether a base
 * can be played was decided when the set was made (an entry whose status is not 0 is refused: -1, the handle is as before, and
 * status[i] carries the entry's status); the moves are checked as there.
 * Start rule: the first searched ply belongs to the side to move of the line's last position -- for a line from the start
 * position that is player white(k) ^ (L & 1), for a base with Black to move and no moves it is Black's player.  The tally stays
 * by White's player, the trace holds the searched plies only, and num_steps, temperature_switch and outcome_gate count from the
 * first searched ply.  The game's chain holds one or two empty records in front of a base where the start rule needs them (they
 * encode as zero planes, and no repetition scan passes the base): the slot's ply is the chain index of its position, not a move
 * count.
 * sc_selfplay_get_opening_fen: the base of the line of handle-local game `game` as sc_positions_fen prints it; returns its
 * length, 0 (and an empty text) for a line from the start position.
 * sc_selfplay_write_trace_json writes such a game's base as "fen": "..." behind "steps" and in front of "opening";
 * sc_selfplay_encode_traces refuses the game, as it refuses every game that did not start from the start position. */
int sc_selfplay_set_openings_from(sc_selfplay*, int n_lines, const sc_positions* bases, const int32_t* base_idx, const uint16_t* moves,
                                  const uint32_t* move_off, int32_t* status);
int sc_selfplay_get_opening_fen(sc_selfplay*, int game, char* buf, int cap);
/* Match play against an outside opponent (the reference's `play --black-type stockfish`, src/play.rs:38-59, 89-142): the handle
 * searches the engine's plies, the opponent's moves come from the host and are played on the device in many slots at once.
 * sc_selfplay_set_external: before the first enqueue, on a handle with rollout_factor = 0 and outcome_gate = -1 (the opponent is
 * never handed a finished position: the reference checks the outcome after every ply).  engine (or NULL: the handle's) evaluates
 * the engine's plies, synth_salt is the synthetic evaluators' player.  colours: 0 the engine is White in every game, 1 White in the
 * even games of the handle and Black in the odd ones, 2 Black in every game.  Any n_games >= 1 on any n_slots, with or without a
 * trace ring; a finished game's slot goes on with the next game, and any game may start at any ply boundary.  On such a handle
 * sc_selfplay_enqueue_sims, _enqueue_interleaved, _run, _set_players, _set_match and _set_openings[_from] return -1.
 * A round: sc_selfplay_external_wait -> the opponent's answers -> sc_selfplay_push_moves, repeated while slots wait (a game that
 * starts with the opponent as White appears in a second pass), then sc_selfplay_external_search.
 * sc_selfplay_external_search: -1 while a slot waits for the opponent (the count of the last sc_selfplay_external_wait; where moves
 * were pushed since, or on a fresh handle, the wait kernel runs first and the call completes the handle's work).  Otherwise it
 * enqueues one searched ply of every live game -- rollout_num simulation steps in the handle's launch form, the expansions that end
 * the ply, the boundary kernels that count finished games and start the next -- and does not synchronise: two handles with
 * own_stream = 1 can be overlapped.  sc_selfplay_get_stats().games_active == 0 is the end of the match.
 * sc_selfplay_external_wait: completes the handle's work; returns the number n of slots that wait for the opponent, in ascending
 * slot order.  slots / games (handle-local indices) / plies (from the start position) [cap]; fens: n zero-terminated texts, the
 * text of sc_selfplay_get_fen, entry i at fen_off[i], fen_off[n] the bytes used; moves: each waiting game's moves so far, from its
 * live trace row (for `position startpos moves ...`), entry i at move_off[i] .. move_off[i + 1].  Any output may be NULL; n > cap
 * or too small a text or move buffer returns -1 and writes nothing.
 * sc_selfplay_push_moves: plays moves[i] in slot slots[i] on ANY handle whose listed slots stand at a ply boundary (sim = 0, a fresh
 * one-node root: after sc_selfplay_set_position, or between two plies), an interactive one-slot handle included.  Completes the
 * pending work first.  status[i] (may be NULL): 0 the game goes on, 1 this move ended it (outcome, num_steps), -1 the move is not
 * legal there, -2 the slot does not stand at such a boundary or, on an external handle, the engine is to move; a refused entry
 * changes nothing.  Returns the number of refused entries; -1 for a slot out of range or listed twice.  n = 0 is fine.  On an
 * external handle the boundary kernels run behind the moves: a game ended by a pushed move is counted and its slot refilled.
 * The pushed ply is recorded as the reference records an outside player's ply: children = all legal moves in the generator's
 * order, visit count 1 on the move played and 0 elsewhere, every value 0.
 * sc_selfplay_match_tally serves an external handle with a = the engine and b = the opponent; sc_selfplay_poll, _get_trace,
 * _write_trace_json, _traces_json, _write_pgn (`white` names the engine), _get_fen and _get_slot work unchanged on its games.
 * sc_selfplay_encode_traces accepts these games: the opponent's plies carry one-hot visit counts, as the reference's traces of
 * such games do. */
int sc_selfplay_set_external(sc_selfplay*, sc_engine* engine_or_null, uint64_t synth_salt, int colours);
int sc_selfplay_external_search(sc_selfplay*);
int sc_selfplay_external_wait(sc_selfplay*, int cap, int32_t* slots, int32_t* games, int32_t* plies, char* fens, uint64_t fens_cap,
                              uint32_t* fen_off, uint16_t* moves, uint32_t moves_cap, uint32_t* move_off);
int sc_selfplay_push_moves(sc_selfplay*, int n, const int32_t* slots, const uint16_t* moves, int32_t* status);
/* Plays moves[i] in slot slots[i] and KEEPS the searched subtree below that move: the chosen root child becomes the root, the rest
 * of the node pool and of the tree's position records is compacted away on the device (one workgroup per listed slot), and the
 * next sc_selfplay_enqueue_sims goes on from it.  The tree afterwards is, array for array, what a fresh search from the position
 * after the move holds after as many simulations as the child had visits (no root noise); an unvisited child, or a root that was
 * never searched, gives a one-node root.  The call has sc_selfplay_push_moves's shape: it completes pending work first, a slot out
 * of range or listed twice returns -1, n = 0 is fine, it returns the number of refused entries and a refused entry changes
 * nothing but its status.  status[i] (may be NULL): 0 the game goes on, 1 the move ended it (outcome under the handle's
 * outcome_gate, num_steps: the rules of a searched ply), -1 the move is not playable there -- not among the root's children, or,
 * root not searched, not among the legal moves --, -2 the slot is not active, has a simulation in flight or holds no tree of this
 * search.  The trace step of the ply is what the end of a searched ply records (the real visit distribution, whichever move is
 * played); on a root that was not searched, sc_selfplay_push_moves's one-hot step.  kept (may be NULL) int32 [n][3]: n_nodes, n_exp
 * and the new root's visit count after the call (zeros where status is not 0).
 * Returns -1 on an external handle (its plies end on the device) and on a handle with rollout_factor > 0 (that budget is chosen
 * when the root is the leaf, which a kept root never is).  Scratch: 4 bytes per live node of the listed slots, sized from their
 * n_nodes, allocated by the first call, grown on demand and kept on the handle. */
int sc_selfplay_advance(sc_selfplay*, int n, const int32_t* slots, const uint16_t* moves, int32_t* status, int32_t* kept);
int sc_selfplay_timing(sc_selfplay*, int reset, float* ms_total, float* ms_nn, int64_t* nn_launches);
/* Kernel launches per simulation step this handle uses with SC_EVAL_NET (steps bracketed for sc_selfplay_timing always use 3):
 * 1 = the fused step kernel with value_head.ffn.0 inside (whole 64-slot blocks, every workgroup resident, and no other
 *     stream of this process running that form on the device: its workgroups wait for each other inside the launch),
 * 2 = the fused step kernel + the value FC launch, 3 = search, network tower and value FC as separate launches.
 * All three play bit-identical games.  0 for handles without a network. */
int sc_selfplay_launches_per_step(const sc_selfplay*);

/* Trace of a finished game = the reference's Trace<M,O> (src/trace.rs:5-9) in SoA form.
 * Call with NULL arrays to query sizes first.  child_off has n_steps+1 entries. */
typedef struct {
    int32_t n_steps;
    int32_t n_children_total;
    int32_t has_outcome;   /* 0: outcome null (src/trace.rs:7), 1: set */
    int32_t termination;   /* src/chess.rs:88-99 */
    int32_t winner;        /* 1 white, 0 black, -1 none */
    uint64_t game_id;
} sc_trace_info;
/* Returns 0 ok, 1 the game has not finished yet, 2 its trace is no longer on the device (ring row overwritten by a
 * later game, or released by sc_selfplay_poll), < 0 error. */
int sc_selfplay_get_trace(sc_selfplay*, int game /*0..n_games-1*/, sc_trace_info* info, uint16_t* step_move,
                          float* step_q, int32_t* child_off, uint16_t* child_move, int32_t* child_n, float* child_q,
                          float* child_uct);
/* Streaming drain: completes the enqueued work, then returns the number of games (written to
 * finished_games[0..cap), handle-local indices usable with sc_selfplay_get_trace / _write_trace_json) that have finished
 * since they were last reported.  With trace_hold the traces reported by the PREVIOUS call are released first (their ring
 * rows become free for new games), so the host reads each batch between two polls.  < 0: error. */
int sc_selfplay_poll(sc_selfplay*, int32_t* finished_games, int cap);
/* Training tensors of finished games, from the trace ring rows in place (see sc_encode_steps_device for the outputs, layouts,
 * the scatter_add_ rule and the stream contract).  games[0..n): handle-local game indices (host).  ply_off (host, n+1) receives
 * the plies of game i: [ply_off[i], ply_off[i+1]); call with every output (status included) NULL to get the sizes only.
 * Readiness as sc_selfplay_get_trace: returns 1 if a requested game has not finished, 2 if its row has been overwritten or
 * released (2 wins over 1); nothing is enqueued then.  If every requested game was reported by sc_selfplay_poll and is held
 * (trace_hold), the rows are final and are read without waiting for the handle's stream (simulation steps enqueued before
 * may still run); the next sc_selfplay_poll waits for this work before it releases them.  Otherwise the handle's work is
 * completed first, and the handle's later steps wait on the device for this work.  A poisoned handle refuses with
 * SC_ERR_HANDOFF. */
int sc_selfplay_encode_traces(sc_selfplay*, int n, const int32_t* games, int apply_mirror, int layout, void* stream, uint32_t* ply_off,
                              void* boards, void* meta, float* dist, float* dist_legal, uint16_t* legal_idx, int32_t* n_legal,
                              int32_t* status);
/* Writes the reference's trace JSON (src/trace.rs:23-32; serde_json pretty, keys "outcome","steps").  A game that started from a
 * non-empty opening line (sc_selfplay_set_openings) gets a third key after "steps": "opening": ["e2e4", ...], the line's moves. */
int sc_selfplay_write_trace_json(sc_selfplay*, int game, const char* path);

/* Finished games as PGN, written (append = 0) or appended to `path`: one sc_moves_to_san_device_from call renders the batch.
 * games[0..n): handle-local indices.  A game's moves are its opening line (sc_selfplay_get_opening) and the trace's played moves,
 * from the line's base where it has one (sc_selfplay_get_opening_fen): then [SetUp "1"] and [FEN "..."] are written and the move
 * numbers start at the base's.  Headers: Event, Round (the game id), White, Black (the names given, "?" for NULL; on a handle with
 * sc_selfplay_set_match colours = 1 `white` names player a and the odd games carry the names exchanged), Result (* without an
 * outcome, 1-0, 0-1, 1/2-1/2), Termination (the reference's enum name, with an outcome).  Movetext lines of at most 80 columns, the
 * result at the end, a blank line behind every game.  Readiness as sc_selfplay_get_trace: returns 1 if a game has not finished,
 * 2 if its row is gone (2 wins over 1); nothing is written then. */
int sc_selfplay_write_pgn(sc_selfplay*, int n, const int32_t* games, const char* path, int append, const char* white, const char* black,
                          const char* event);

/* tests / NNPlayer::bestmove (src/play.rs:241-288) support: current search tree of a slot in
 * allocation order (root = 0; children of a node contiguous).  Arrays may be NULL; returns n_nodes. */
int sc_selfplay_get_tree(sc_selfplay*, int slot, int cap, int32_t* n, float* q, float* uct, float* prior, uint16_t* move,
                         int32_t* first_child, int32_t* n_child);
int sc_selfplay_get_slot(sc_selfplay*, int slot, int32_t* ply, int32_t* sim, int32_t* status, uint64_t* game_id,
                         int32_t* last_path /*cap 1024*/, int32_t* last_path_len);
/* replace the root noise used by the NEXT simulation of `slot` (external_noise mode); noise[n] */
int sc_selfplay_set_noise(sc_selfplay*, int slot, const float* noise, int n);
int sc_selfplay_get_noise(sc_selfplay*, int slot, float* noise, int cap);
/* start slot from a given move list instead of the initial position (sc_search / chess_play_new, src/lib.rs:161-232); from a
 * position given as FEN: sc_selfplay_set_position_from */
int sc_selfplay_set_position(sc_selfplay*, int slot, const uint16_t* moves, int n_moves);
/* per-call search options of chess_play_mcts(state, rollout, cpuct, noise) (src/lib.rs:233-247): applies to the
 * simulations enqueued after the call */
int sc_selfplay_set_search(sc_selfplay*, float cpuct, float epsilon, int with_noise);

/* One search as a single call: NNPlayer::bestmove's mcts::mcts (src/play.rs:241-252) / chess_play_mcts (src/lib.rs:233-247).
 * Runs `rollout` simulations from the position reached by `moves` (fresh tree, epsilon 0.15) and returns the number of root
 * children (< 0: error); child_move / child_n / child_q / child_prior receive up to `cap` of them in python-chess move
 * order (any may be NULL), *root_q the root's value sum.  The engine keeps ONE one-slot handle for these calls and reuses it
 * (every call restarts from a one-node tree with its own options and seed: the result does not depend on earlier calls), so
 * calls on one engine must not overlap; to keep the tree between moves use a handle of your own (sc_selfplay_set_position +
 * sc_selfplay_enqueue_sims + sc_selfplay_get_tree). */
int sc_search(sc_engine*, const uint16_t* moves, int n_moves, int rollout, float cpuct, int with_noise, uint64_t seed, int cap,
              uint16_t* child_move, int32_t* child_n, float* child_q, float* child_prior, float* root_q);

/* The same from a base (sc_positions_from_fen): entry i of `bases` followed by `moves`.  bases == NULL: the start position, and
 * the call is its sibling without _from.  An entry whose status is not 0 is refused (-1): nothing can be searched from a position
 * that cannot be played or where the game is over.
 * sc_selfplay_set_position_from: hist[0] of the slot is the base; the slot's ply and start ply stay counts of the moves AFTER the
 * base, history planes older than the base are zero, repetitions and the fifty-move count start at the base.  The moves are not
 * checked, as with sc_selfplay_set_position (sc_encode_positions_from reports an illegal one).
 * sc_selfplay_get_fen: python-chess's Board.fen() of the slot's current position (the root of its tree), whatever the slot
 * started from; the ep square is printed only if a legal en-passant capture exists, which a lane of a small kernel decides.
 * Returns the length, writes at most cap bytes with the final zero. */
int sc_selfplay_set_position_from(sc_selfplay*, int slot, const sc_positions* bases, int i, const uint16_t* moves, int n_moves);
int sc_search_from(sc_engine*, const sc_positions* bases, int i, const uint16_t* moves, int n_moves, int rollout, float cpuct,
                   int with_noise, uint64_t seed, int cap, uint16_t* child_move, int32_t* child_n, float* child_q, float* child_prior,
                   float* root_q);
int sc_selfplay_get_fen(sc_selfplay*, int slot, char* buf, int cap);

/* ------------------------------------------------------------------ the search report */
/* What a search found, read from the trees where they lie: one kernel launch for every requested slot, one copy to the host.
 * Entry i reports slot slots[i] (slots == NULL: slot i), n entries.  All pointers are host pointers; any output may be NULL.
 * The call completes the handle's pending work first (the expansion and backup of the last enqueued simulation, as
 * sc_selfplay_get_tree does): the report sees a fully backed-up tree.  It works on every kind of handle -- self-play, match,
 * external, an interactive one-slot handle -- and changes nothing the search reads: a handle that is reported on between
 * enqueues plays bit-identical games.  A slot listed twice or out of range returns -1 and writes nothing; n == 0 is fine; a
 * poisoned handle refuses with SC_ERR_HANDOFF.
 * Lines: the root's child i has rank #{ j : N[j] > N[i], or N[j] == N[i] and j < i } -- visits descending, then the generator's
 * order, so rank 0 is the FIRST most-visited child (mcts::step, src/mcts.rs:309-311; children without a visit are ranked like
 * the rest).  Line r of an entry, 0 <= r < n_lines = min(multipv, children of the root), is the child of rank r and its
 * principal variation: from a node the walk goes to the most-visited child, ties to the lowest index, while the node is
 * expanded, has children and that child has a visit; it never takes more than 1024 moves (the search's depth limit).
 * Per line, row i * multipv + r: line_child the child's index among the root's children, line_n / line_w / line_prior its visit
 * count, value sum (White's point of view, as the search adds it up) and cached prior, line_len the FULL length of the walk,
 * line_end what the last node is -- 0 open (unexpanded, or no visited child), 1 / 2 / 3 a terminal whose game is drawn / won by
 * White / won by Black, 4 cut at the depth limit -- and pv[(i * multipv + r) * pv_cap ..] the first min(line_len, pv_cap) moves.
 * Nothing else is written: rows from n_lines on, and the moves behind min(line_len, pv_cap), keep what the arrays held.
 * Per entry, info[i]: status / ply / sim / n_nodes of the slot, n_root_children, root_children_n the sum of the root children's
 * visits, root_n / root_w the root's own, turn the side to move at the root (1 White, 0 Black; -1 where the slot holds no game)
 * and n_lines -- 0 where the slot is idle or finished, the root is unexpanded (sim == 0), terminal or without children.
 * sc_selfplay_report_last_timing: measurement aid (tools/report_rate.py) -- HIP-event time of the kernel and host time of the
 * whole call, of the calling thread's last sc_selfplay_report. */
struct sc_report_slot {
    int32_t status, ply, sim, n_nodes, n_root_children, root_children_n, root_n, turn, n_lines, pad;
    float root_w;
};
typedef struct sc_report_slot sc_report_slot;
int sc_selfplay_report(sc_selfplay*, int n, const int32_t* slots /* NULL: slots 0..n-1 */, int multipv /* 1..224 */, int pv_cap /* 0..1024 */,
                       sc_report_slot* info /*[n]*/, int32_t* line_child, int32_t* line_n, float* line_w, float* line_prior,
                       int32_t* line_len, int32_t* line_end /* each [n][multipv] */, uint16_t* pv /*[n][multipv][pv_cap]*/);
int sc_selfplay_report_last_timing(float* kernel_ms, float* total_ms);

/* test aid: find_max (src/mcts.rs:78-88, Iterator::max_by: the LAST maximum wins) as the descent computes it, on n <= 256
 * caller-provided finite values: out[0] = the one-round form used for nodes with <= 64 children (-2 if n > 64),
 * out[1] = the four-round (value, index) form used for wider nodes. */
int sc_debug_find_max(int device_id, const float* values, int n, int32_t* out2);
/* test aid: the end-of-ply move choice (mcts::step, src/mcts.rs:298-317; with tie_random NNPlayer::bestmove, src/play.rs:268-277)
 * on caller-provided visit counts, by the device function the self-play kernels call: one wave per case, all cases in one
 * launch.  Case c: n_act[c * 224 .. + nc[c]) the children's counts (1 <= nc[c] <= 224, counts in [0, 60000]), temperature[c] >= 0
 * the temperature already resolved for the ply (at most 64 distinct values per call), u[c] in [0, 1) the uniform draw.
 * choice_out[c] = the chosen child; total_out[c] = the f32 sum of the weights N^(1/temperature) (0 at temperature 0).  The
 * weights come from tables the host fills with its libm's powf, one per temperature, exactly as sc_selfplay_create does for a
 * handle.  A total of 0 or infinity makes the reference panic; here an index is returned all the same (recorded behaviour,
 * pinned by the tests). */
int sc_debug_choose_child(int device_id, int n_cases, const int32_t* n_act, const int32_t* nc, const float* temperature,
                          const float* u, int tie_random, int32_t* choice_out, float* total_out);
/* test aid: makes the NEXT one-launch steps of the handle wait for arrivals that never come (the in-launch hand-off's target is
 * raised by `missing` arrivals per block), to show on hardware that the wait is bounded: every workgroup gives up after ~0.2 s,
 * the launch ends and error_flags carries bit 32.  The handle's results are invalid afterwards and it refuses further work
 * (SC_ERR_HANDOFF).  No effect (returns 1) on a handle that does not use the one-launch form. */
int sc_selfplay_debug_break_handoff(sc_selfplay*, int missing);
/* test aid: forget that an in-launch hand-off has failed on the device (after such a failure new handles get the two-launch
 * step for the rest of the process; tests that provoke the failure restore the default with this).  0 = a record was cleared. */
int sc_debug_clear_handoff_failure(int device_id);
/* developer aid: stamps of the last launch, out[n_slots][32]: 0..7 the search's cycle stamps (tools/dbg_cycles.py); 24..27 the
 * one-launch step's phases on the 100 MHz wall clock (kernel entry, leaf selected, network done, value-FC tile done: bench.py's
 * per-phase split); the rest unused */
int sc_selfplay_debug_cycles(sc_selfplay*, int enable, unsigned long long* out);

/* utility: trace-file JSON writer on caller-provided arrays (no GPU needed) */
int sc_trace_write_json(const char* path, const sc_trace_info* info, const uint16_t* step_move, const float* step_q,
                        const int32_t* child_off, const uint16_t* child_move, const int32_t* child_n,
                        const float* child_q, const float* child_uct);
/* ------------------------------------------------------------------ trace files written on the device */
/* Search records -> the text of trace files, formatted by kernels: the bytes are EXACTLY those of sc_trace_write_json /
 * sc_selfplay_write_trace_json (key order, two-space pretty form, null for a non-finite value, -0.0, "fen" and "opening" behind
 * "steps", [] for no steps or no children, no trailing newline).  One call formats n games; the text of game g is
 * text[text_off[g] .. text_off[g + 1]) and comes to the host in one copy.  The work runs on a non-blocking stream of the
 * writer's own and the calls return when the text is on the host.
 *
 * sc_trace_format_f32: the number formatter alone, on the host (no GPU is needed; the kernels compile the same source, which
 * uses integer arithmetic only): text[i][0 .. len[i]) is the shortest decimal that reads back as the float64 v[i] widens to, in
 * ryu's pretty layout as the host writer prints it ("null" for a non-finite value); len[i] <= 24, no final zero.
 * sc_traces_format: host arrays in, host text out.  info [n] (n_steps must equal step_off[g + 1] - step_off[g]; has_outcome,
 * termination, winner as sc_trace_info), step_off [n + 1] from 0, step_move / step_q one per step, child_off [steps + 1] from 0
 * into child_move / child_n / child_q / child_uct (at most SC_MAX_MOVES children per step, at most 4000 steps per game),
 * open_off [n + 1] into opening (NULL: no game has an "opening" member), fens [n] (NULL, or NULL entries: no "fen" member; the
 * text must need no JSON escape).  text_off [n + 1] is always filled.  text == NULL is the sizing call.  If cap <
 * text_off[n] the call returns -1 and writes no text.  n == 0 is valid.  Argument errors are found before a device is looked for
 * (-3: no HIP device).
 * sc_selfplay_traces_json: the same for finished games of a handle, games[0..n) handle-local indices, read from the trace ring
 * rows IN PLACE; "opening" and "fen" come from the handle's lines.  Readiness as sc_selfplay_encode_traces: returns 1 if a
 * requested game has not finished, 2 if its row has been overwritten or released (2 wins over 1); nothing is written then.  If
 * every requested game is held (trace_hold, reported by the last sc_selfplay_poll) the rows are read without waiting for the
 * handle's stream, while its simulation steps run; the call has finished reading them when it returns, so the next
 * sc_selfplay_poll may release them.  Otherwise the handle's work is completed first.  A poisoned handle: SC_ERR_HANDOFF.
 * sc_selfplay_write_traces_json: the above, and game i's text written to paths[i].  The pinned staging buffer belongs to the
 * handle and grows on demand.
 * sc_traces_format_last_timing: measurement aid (tools/trace_write_rate.py) -- HIP-event time of the counting pass and of the
 * emitting passes (with their scans) of the calling thread's last call of the three above. */
int sc_trace_format_f32(int n, const float* v, char* text /*[n][24]*/, uint8_t* len);
int sc_traces_format(int device_id, int n, const sc_trace_info* info, const uint32_t* step_off, const uint16_t* step_move,
                     const float* step_q, const uint32_t* child_off, const uint16_t* child_move, const int32_t* child_n,
                     const float* child_q, const float* child_uct, const uint32_t* open_off, const uint16_t* opening,
                     const char* const* fens, char* text, uint64_t cap, uint64_t* text_off);
int sc_selfplay_traces_json(sc_selfplay*, int n, const int32_t* games, char* text, uint64_t cap, uint64_t* text_off);
int sc_selfplay_write_traces_json(sc_selfplay*, int n, const int32_t* games, const char* const* paths);
int sc_traces_format_last_timing(float* count_ms, float* emit_ms);

/* utility: UCI text of a move (src/chess.rs:513-519); returns strlen */
int sc_move_uci(uint16_t move, char* buf8);
/* libsmartchess.chess_encode_move(turn, move) (reference src/lib.rs:37-44; src/chess.rs:544-550, queenmoves.rs,
 * knightmoves.rs, underpromotions.rs): action index in [0, 4672) of `move` for the side to move, -1 if it has none.
 * Host function, needs no GPU. */
int sc_move_index(uint16_t move, int white_to_move);

#ifdef __cplusplus
}
#endif
#endif
