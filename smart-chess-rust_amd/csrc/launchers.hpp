// launchers.hpp -- host entry points of the kernel translation units.  A kernel family's arguments travel as blocks, passed to the
// kernels by value (*_types.hpp); the stream comes last.
#pragma once
#include <hip/hip_runtime.h>

namespace scl {
// scan_kernels.hip: the exclusive scan of d_in[0 .. n) into d_out[0 .. n) and the total into *d_total, modulo 2^32; nothing for n == 0.
// d_tile_sum: scratch of (n + SCAN_TILE - 1) / SCAN_TILE words, SCAN_TILE being the counts per workgroup (256 threads x 4).  Three
// launches on s.  (Ahead of the type headers: merge_types.hpp lays out its workspace with SCAN_TILE)
constexpr int SCAN_TILE = 1024;
void exclusive_scan_u32(uint32_t n, const uint32_t* d_in, uint32_t* d_tile_sum, uint32_t* d_out, uint32_t* d_total, hipStream_t s);
}  // namespace scl

#include "mcts_types.hpp"
#include "nn_types.hpp"
#include "score_types.hpp"
#include "batch_types.hpp"
#include "merge_types.hpp"
#include "encode_types.hpp"
#include "perft_types.hpp"
#include "report_types.hpp"
#include "trace_types.hpp"
#include "trace_write_types.hpp"
#include "advance_types.hpp"

struct sc_fen_fields;   // include/sc_engine.h

namespace scl {
// mcts_kernels.hip (compiled with -ffp-contract=off)
void init_slots(const sc::SpParams& p, const sc::MatchLines& lines, hipStream_t s);
void mcts(const sc::SpParams& p, int do_expand, int do_select, hipStream_t s);
void synth_eval(const sc::SpParams& p, hipStream_t s);
void debug_find_max(const float* d_u, int n, int* d_out, hipStream_t s);
void debug_choose_child(int n_cases, const int32_t* d_n_act, const int32_t* d_nc, const float* d_temperature, const float* d_u, int tie_random,
                        const float* d_w, const int32_t* d_w_off, int w_max, int32_t* d_choice, float* d_total, hipStream_t s);
void set_position(const sc::SpParams& p, int slot, const uint16_t* d_moves, int n_moves, hipStream_t s, const sc::Position* d_base = nullptr);
void match_boundary(const sc::SpParams& p, const sc::MatchLines& lines, hipStream_t s);   // match recycling: count the games that ended, start the next ones
// sc_selfplay_set_openings: replay and check n_lines move lists into their records (rec_off as sc::MatchLines::off) -> status [n_lines]
// With bases, a line that has one starts behind as many empty records as rec_off leaves room for in front of it
// (sc_selfplay_set_openings_from)
void open_lines(int n_lines, const uint16_t* d_moves, const uint32_t* d_move_off, sc::Position* d_tab, const uint32_t* d_rec_off,
                int32_t* d_status, const sc::Bases& bases, hipStream_t s);
void match_tally(const int32_t* d_tally, int n_slots, long long* d_out, hipStream_t s);   // [n_slots][2][4] -> [8]
// external_kernels.hip (compiled with -ffp-contract=off): an outside opponent.  external_mode: 0, or 1 + colours of
// sc_selfplay_set_external.  push_moves: entry i plays d_moves[i] in slot d_slots[i] -> d_status[i] (-2 / -1 / 0 / 1).
// external_boundary: count the games that ended, draw the next ones in slot order, start them (three launches).  external_wait: the slots that wait for the
// opponent in slot order -> *d_count, and per entry the slot, its root record, its ep bit and {game, ply, trace row, plies recorded}
void push_moves(const sc::SpParams& p, int n, const int32_t* d_slots, const uint16_t* d_moves, int32_t* d_status, int external_mode,
                hipStream_t s);
void external_boundary(const sc::SpParams& p, int external_mode, hipStream_t s);
void external_wait(const sc::SpParams& p, int external_mode, int32_t* d_list, int32_t* d_count, sc::Position* d_recs, int32_t* d_ep_legal,
                   int4* d_info, hipStream_t s);
// advance_kernels.hip (compiled with -ffp-contract=off): entry i plays a.moves[i] in slot a.slots[i] and keeps the subtree below the
// move (sc_selfplay_advance); the argument block is advance_types.hpp's.  One workgroup per entry; nothing for a.n == 0
void advance(const sc::SpParams& p, const scad::AdvanceArgs& a, hipStream_t s);
// encode_kernels.hip (compiled with -ffp-contract=off); the argument blocks are encode_types.hpp's
void encode_positions(const sc::GameWalk& w, const sc::PlyRows& rows, int32_t* outcome, hipStream_t s);   // one position per "game"
// training tensors (sc_encode_steps, sc_encode_steps_device, sc_selfplay_encode_traces): see encode_kernels.hip
void ply_index(const sc::PlyGroup& g, const sc::PlyIndex& idx, const sc::RingPlies& ring, hipStream_t s);
// the walk alone: boards, castling rights, ep squares and clocks of every ply (keys and flags stay 0), which is all a move
// generation reads (sc_moves_to_san_device)
void replay_walk(const sc::GameWalk& w, hipStream_t s);
// ... and the keys and repetition flags of its n_plies plies: idx and d_ply_moves are those of the group's first ply on
void replay_games(const sc::GameWalk& w, int n_plies, const sc::PlyIndex& idx, const uint16_t* d_ply_moves, hipStream_t s);
void encode_plies(int layout, int n, const sc::Position* d_hist, const sc::PlyIndex& idx, const sc::PlyRows& rows, hipStream_t s);
void steps_dist(int n, const sc::PlyMoves& m, const sc::Children& c, const sc::PlyIndex& idx, const sc::RowOut& o, int32_t* status,
                hipStream_t s);
void status_final(int n, int32_t* status, hipStream_t s);
// san_kernels.hip: SAN tokens -> moves and the parser's status per game (sc_encode_san_device), and steps_dist for rows whose
// children are the legal moves with count 1 on the played move
void san_parse(int n_games, const uint64_t* d_tokens, const uint32_t* d_tok_off, uint16_t* d_moves, int32_t* d_status,
               const sc::Bases& bases, hipStream_t s);
void san_dist(int n, const sc::PlyMoves& m, const sc::RowOut& o, hipStream_t s);
// san_write_kernels.hip: moves -> SAN tokens, one wavefront per ply of a walked group (sc_moves_to_san_device); d_status holds
// k_steps_dist's keys (sc::STATUS_NONE at first, status_final behind it); san_clip zeroes a game's tokens from its first failing ply on
void san_write(int n, const sc::Position* d_hist, const sc::PlyIndex& idx, const uint16_t* d_ply_moves, uint64_t* d_tokens,
               int32_t* d_status, hipStream_t s);
void san_clip(int n, const sc::PlyIndex& idx, const int32_t* d_status, uint64_t* d_tokens, hipStream_t s);
// fen_kernels.hip: raw FEN fields -> validated records and their status (sc_positions_from_fen); the ep bit of Board.fen()
void fen_positions(int n, const sc_fen_fields* d_fields, const int32_t* d_syntax, sc::Position* d_out, int32_t* d_status, hipStream_t s);
void fen_ep_legal(int n, const sc::Position* d_rec, int32_t* d_ep_legal, hipStream_t s);
// trace_kernels.hip: trace files read on the device (sc_traces_read).  trace_count: per file the status, the counts, the outcome and
// the "fen" member; trace_emit: the packed arrays, at the bases the exclusive scans of the counts give; trace_status: the reader's
// codes over the encoder's (sc_traces_encode_device)
void trace_count(const sctr::Text& t, const sctr::Files& f, hipStream_t s);
void trace_emit(const sctr::Text& t, const sctr::Files& f, const sctr::Packed& p, hipStream_t s);
void trace_status(int n, const int32_t* d_over, int32_t* d_status, hipStream_t s);
// trace_write_kernels.hip: trace files written on the device (sc_traces_format, sc_selfplay_traces_json); the argument blocks are
// trace_write_types.hpp's.  trace_write_count: the bytes of every ply into d_seg_len[p.seg[.]] (the frames' lengths are the
// host's; exclusive_scan_u32 then gives o.seg_off).  trace_write_emit: the frames and the plies of a group of games into o.text
void trace_write_count(const sctw::Plies& p, const sctw::Steps& s, uint32_t* d_seg_len, hipStream_t st);
void trace_write_emit(const sctw::Plies& p, const sctw::Steps& s, const sctw::Frames& f, const sctw::Out& o, hipStream_t st);
// nn_kernels.hip
const char* nn_init();  // sets kernel attributes; returns error text or nullptr
void tower(const scnn::TowerArgs& a, hipStream_t s);
void value_fc1(const scnn::Fc1Args& a, hipStream_t s);
// step_kernels.hip: search wave + tower in one launch (slot g = position g; a.n_pos must equal p.n_slots)
const char* step_init();
int step_blocks_per_cu(const scnn::NetLayout& net);
void step(const scnn::TowerArgs& a, const sc::SpParams& p, int do_expand, hipStream_t s);
void value_finish(const scnn::VfinArgs& a, hipStream_t s);
// score_kernels.hip (compiled with -ffp-contract=off): losses / agreement per position from the tower's log-probability rows,
// and the [P] -> summary reduction (sc_score_positions, sc_compare_engines)
void score_positions(const scsc::ScoreArgs& a, hipStream_t s);
void compare_rows(const scsc::CompareArgs& a, hipStream_t s);
void score_summary(const scsc::SummaryArgs& a, hipStream_t s);
// batch_kernels.hip: rows of the compact training tensors, chosen by index -> a trainer-layout minibatch (sc_gather_batch)
void gather_batch(const scbt::GatherArgs& a, hipStream_t s);
// merge_kernels.hip: identical rows of the compact training tensors -> one row each, targets averaged (sc_merge_positions); a.n_in > 0.
// Enqueues everything on s; an error that is not HIP's own is named in *why
hipError_t merge_positions(const scmg::MergeArgs& a, hipStream_t s, const char** why);
// perft_kernels.hip: perft on the device (sc_perft); the argument blocks are perft_types.hpp's.  perft_roots: the entries of a chunk
// replayed into level 0, their status and the divide rows' moves.  perft_count: legal moves per node (perft.hip scans them into
// d_off[0 .. n], the total last, with exclusive_scan_u32).  perft_expand: the children of a piece of a level into the next level.
// perft_leaf: the last level -- counts (with lo.kinds: the kinds of every node's moves too) and their sums by root move
void perft_roots(const scpf::RootArgs& a, hipStream_t s);
void perft_div_ones(int n, const int32_t* d_n_div, unsigned long long* d_div_nodes, hipStream_t s);   // depth 1: a leaf per legal move
void perft_count(const scpf::Level& lv, uint32_t* d_cnt, hipStream_t s);
void perft_expand(const scpf::ExpandArgs& a, hipStream_t s);
void perft_leaf(const scpf::Level& lv, const scpf::LeafOut& lo, const scpf::Totals& t, hipStream_t s);
// report_kernels.hip (compiled with -ffp-contract=off): the search report (sc_selfplay_report); the argument block is
// report_types.hpp's.  One wavefront per (entry, line): a.n * a.multipv workgroups of 64 threads; nothing for a.n == 0
void report(const scrp::ReportArgs& a, hipStream_t s);
}  // namespace scl
