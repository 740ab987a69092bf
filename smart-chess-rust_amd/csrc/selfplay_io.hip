// selfplay_io.hip -- host side of libsc_engine.so: what the host reads from and writes to a self-play handle (drain, traces,
// tree / slot / noise / position accessors) and sc_search, which drives a one-slot handle through them.
#include <string.h>

#include "host_common.hpp"
#include "san_tokens.hpp"
#include "trace_json.hpp"

bool row_held(const sc_selfplay* sp, int row, uint64_t want_id) {
    return sp->p.trace_hold && sp->reported[(size_t)row] == want_id + 1 &&
           std::find(sp->to_release.begin(), sp->to_release.end(), row) != sp->to_release.end();
}
RowState row_state(const sc_selfplay* sp, int row, uint64_t want_id, const sc::TraceHdr& h) {
    if (h.state == sc::TR_FREE) return sp->reported[(size_t)row] > want_id ? ROW_GONE : ROW_NOT_FINISHED;
    if (h.game_id > want_id) return ROW_GONE;
    return h.game_id < want_id || h.state != sc::TR_DONE ? ROW_NOT_FINISHED : ROW_READY;
}

// a PGN tag pair; quotes and backslashes of the value escaped
static std::string pgn_tag(const char* name, const std::string& value) {
    std::string o = std::string("[") + name + " \"";
    for (char c : value) {
        if (c == '"' || c == '\\') o += '\\';
        o += c;
    }
    return o + "\"]\n";
}
// one line of movetext -> lines of at most 80 columns, broken at blanks
static std::string pgn_wrap(const std::string& text) {
    std::string o;
    size_t col = 0;
    for (size_t i = 0; i < text.size();) {
        size_t e = text.find(' ', i);
        if (e == std::string::npos) e = text.size();
        if (col && col + 1 + (e - i) > 80) {
            o += '\n';
            col = 0;
        } else if (col) {
            o += ' ';
            col++;
        }
        o.append(text, i, e - i);
        col += e - i;
        i = e + 1;
    }
    return o + "\n";
}

// the opening of an accessor of one slot: the handle quiesced (no latch), the slot's control block read
static int sp_read_ctl(sc_selfplay* sp, int slot, sc::GameCtl* c) {
    TRY(sp_quiesce(sp, false));
    HIPOK(hipMemcpy(c, sp->p.ctl + slot, sizeof *c, hipMemcpyDeviceToHost));
    return 0;
}

// A finished game's row of the trace ring on the host: the header and the child counts always, of the arrays those named in `want`
// (every vector holds one spare element: data() is never null).  The children are compacted: those of ply i start at child_off[i].
enum { TR_MOVE = 1, TR_Q = 2, TR_CMOVE = 4, TR_CN = 8, TR_CQ = 16, TR_CU = 32, TR_ALL = 63 };
struct TraceRow {
    sc_trace_info info;
    std::vector<int32_t> child_off, cn;   // [n_steps + 1], [n_children_total]
    std::vector<uint16_t> move, cmove;    // [n_steps], [n_children_total]
    std::vector<float> q, cq, cu;
};
// one copy per array for the whole game (rows of 224 entries per ply), compacted on the host: a copy per ply and array cost more
// than the games themselves when many short games stream out
template <class T>
static int read_children(const TraceRow& r, const T* d_rows, std::vector<T>& out) {
    const size_t ns = (size_t)r.info.n_steps;
    std::vector<T> rows(ns * 224 + 1);
    if (ns) HIPOK(hipMemcpy(rows.data(), d_rows, ns * 224 * sizeof(T), hipMemcpyDeviceToHost));
    out.resize((size_t)r.info.n_children_total + 1);
    for (size_t i = 0; i < ns; i++)
        memcpy(out.data() + r.child_off[i], rows.data() + i * 224, (size_t)(r.child_off[i + 1] - r.child_off[i]) * sizeof(T));
    return 0;
}
// 0, 1: the game has not finished, 2: its row is gone, < 0: an error -- the codes of sc_selfplay_get_trace
static int sp_read_trace(sc_selfplay* sp, int game, unsigned want, TraceRow& r) {
    if (!sp || game < 0 || game >= sp->p.total_games) return fail("bad argument");
    const uint64_t want_id = sp->p.first_game_id + (uint64_t)game;
    game %= sp->p.trace_cap;
    if (sp->poisoned) return sp_refuse(sp);
    // A held row is read without waiting for the stream, so a consumer can enqueue the next simulation steps first and fetch /
    // write the finished traces while they run (the copies below are on the NULL stream; the launch stream is non-blocking).
    // Anything else is read from an idle stream.
    if (row_held(sp, game, want_id)) HIPOK(hipSetDevice(sp->device));
    else TRY(sp_quiesce(sp, true));
    const sc::SpParams& p = sp->p;
    sc::TraceHdr h;
    HIPOK(hipMemcpy(&h, p.thdr + game, sizeof h, hipMemcpyDeviceToHost));
    switch (row_state(sp, game, want_id, h)) {
        case ROW_NOT_FINISHED: return fail("game not finished", 1);
        case ROW_GONE: return fail(h.state == sc::TR_FREE ? "trace released or overwritten" : "trace overwritten by a later game (trace_capacity ring)", 2);
        case ROW_READY: break;
    }
    const size_t ns = (size_t)h.n_steps, base = (size_t)game * (size_t)p.num_steps;
    r.child_off.assign(ns + 2, 0);
    if (ns) HIPOK(hipMemcpy(r.child_off.data() + 1, p.t_nchild + base, ns * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < ns; i++) r.child_off[i + 1] += r.child_off[i];
    r.info.n_steps = h.n_steps;
    r.info.n_children_total = r.child_off[ns];
    r.info.has_outcome = h.has_outcome;
    r.info.termination = h.termination;
    r.info.winner = h.winner;
    r.info.game_id = h.game_id;
    r.move.resize(ns + 1);
    r.q.resize(ns + 1);
    if ((want & TR_MOVE) && ns) HIPOK(hipMemcpy(r.move.data(), p.t_move + base, ns * 2, hipMemcpyDeviceToHost));
    if ((want & TR_Q) && ns) HIPOK(hipMemcpy(r.q.data(), p.t_q + base, ns * 4, hipMemcpyDeviceToHost));
    if (want & TR_CMOVE) TRY(read_children(r, p.t_cmove + base * 224, r.cmove));
    if (want & TR_CN) TRY(read_children(r, p.t_cn + base * 224, r.cn));
    if (want & TR_CQ) TRY(read_children(r, p.t_cq + base * 224, r.cq));
    if (want & TR_CU) TRY(read_children(r, p.t_cu + base * 224, r.cu));
    return 0;
}

extern "C" {

int sc_selfplay_get_trace(sc_selfplay* sp, int game, sc_trace_info* info, uint16_t* step_move, float* step_q,
                          int32_t* child_off, uint16_t* child_move, int32_t* child_n, float* child_q, float* child_uct) {
    if (!info) return fail("bad argument");
    TraceRow r;
    TRY(sp_read_trace(sp, game, (step_move ? TR_MOVE : 0) | (step_q ? TR_Q : 0) | (child_move ? TR_CMOVE : 0) | (child_n ? TR_CN : 0) |
                                    (child_q ? TR_CQ : 0) | (child_uct ? TR_CU : 0), r));
    *info = r.info;
    const size_t ns = (size_t)r.info.n_steps, nc = (size_t)r.info.n_children_total;
    if (step_move) memcpy(step_move, r.move.data(), ns * 2);
    if (step_q) memcpy(step_q, r.q.data(), ns * 4);
    if (child_off) memcpy(child_off, r.child_off.data(), (ns + 1) * 4);
    if (child_move) memcpy(child_move, r.cmove.data(), nc * 2);
    if (child_n) memcpy(child_n, r.cn.data(), nc * 4);
    if (child_q) memcpy(child_q, r.cq.data(), nc * 4);
    if (child_uct) memcpy(child_uct, r.cu.data(), nc * 4);
    return 0;
}

int sc_selfplay_poll(sc_selfplay* sp, int32_t* finished_games, int cap) {
    if (!sp || cap < 0 || (cap > 0 && !finished_games)) return fail("bad argument");
    if (sp->poisoned) return sp_refuse(sp);
    TRY(sp_quiesce(sp, true));   // (poisoned by this batch: nothing of it is reported, the games that "finished" are not real)
    const sc::SpParams& p = sp->p;
    // an encode of held rows may still be reading them on its own stream
    if (sp->enc_pending) {
        HIPOK(hipEventSynchronize(sp->enc_ev));
        sp->enc_pending = false;
    }
    // rows handed out by the previous poll go back to the device (the stream is idle: no kernel reads them now)
    for (int row : sp->to_release) {
        const int32_t free_state = sc::TR_FREE;
        HIPOK(hipMemcpy(reinterpret_cast<char*>(p.thdr + row) + offsetof(sc::TraceHdr, state), &free_state, 4, hipMemcpyHostToDevice));
    }
    sp->to_release.clear();
    std::vector<sc::TraceHdr> hdr((size_t)p.trace_cap);
    HIPOK(hipMemcpy(hdr.data(), p.thdr, hdr.size() * sizeof(sc::TraceHdr), hipMemcpyDeviceToHost));
    // oldest games first: a consumer that writes trace{N}.json sees them in the order the reference's jobs would finish
    std::vector<std::pair<uint64_t, int>> fin;
    for (int row = 0; row < p.trace_cap; row++) {
        const sc::TraceHdr& h = hdr[(size_t)row];
        if (h.state == sc::TR_DONE && sp->reported[(size_t)row] != h.game_id + 1) fin.emplace_back(h.game_id, row);
    }
    std::sort(fin.begin(), fin.end());
    int n = 0;
    for (auto& f : fin) {
        if (n >= cap) break;
        finished_games[n++] = (int32_t)(f.first - p.first_game_id);
        sp->reported[(size_t)f.second] = f.first + 1;
        if (p.trace_hold) sp->to_release.push_back(f.second);
    }
    return n;
}

int sc_selfplay_encode_traces(sc_selfplay* sp, int n, const int32_t* games, int apply_mirror, int layout, void* stream, uint32_t* ply_off,
                              void* boards, void* meta, float* dist, float* dist_legal, uint16_t* legal_idx, int32_t* n_legal,
                              int32_t* status) {
    if (!sp || n < 0 || (n > 0 && !games) || !ply_off) return fail("bad argument");
    if (sp->poisoned) return sp_refuse(sp);
    const sc::SpParams& p = sp->p;
    std::vector<int32_t> rows((size_t)std::max(n, 1));
    bool all_held = true;
    for (int i = 0; i < n; i++) {
        const int g = games[i];
        if (g < 0 || g >= p.total_games) return fail("bad argument: game index out of range");
        if (sp_opening(sp, g, nullptr) > 0 || sp_opening_fen(sp, g))
            return fail("encode_traces: game " + std::to_string(g) + " started from an opening line (sc_selfplay_set_openings): training tensors "
                        "need the plies from the start position");
        const int row = g % p.trace_cap;
        rows[(size_t)i] = row;
        all_held = all_held && row_held(sp, row, p.first_game_id + (uint64_t)g);   // the readiness rules of sc_selfplay_get_trace
    }
    if (all_held) HIPOK(hipSetDevice(sp->device));
    else TRY(sp_quiesce(sp, true));
    std::vector<sc::TraceHdr> hdr((size_t)p.trace_cap);
    HIPOK(hipMemcpy(hdr.data(), p.thdr, hdr.size() * sizeof(sc::TraceHdr), hipMemcpyDeviceToHost));
    int not_finished = 0, gone = 0;
    ply_off[0] = 0;
    for (int i = 0; i < n; i++) {
        const sc::TraceHdr& h = hdr[(size_t)rows[(size_t)i]];
        const RowState rs = row_state(sp, rows[(size_t)i], p.first_game_id + (uint64_t)games[i], h);
        gone |= rs == ROW_GONE;
        not_finished |= rs == ROW_NOT_FINISHED;
        ply_off[i + 1] = ply_off[i] + (uint32_t)std::max(h.n_steps, 0);
    }
    if (gone) return fail("trace released or overwritten (trace_capacity ring)", 2);
    if (not_finished) return fail("game not finished", 1);
    if (!boards && !meta && !dist && !dist_legal && !legal_idx && !n_legal && !status) return 0;   // sizing call
    if (!status) return fail("bad argument: status is required");
    const DevEncodeOut o{layout, boards, meta, dist, dist_legal, legal_idx, n_legal, status};
    TRY(check_device_outputs(o, sp->device));
    if (n == 0) return 0;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    TRY(encode_device_core(sp->device, n, ply_off, EncodeSrc::ring(rows.data(), &p), apply_mirror, o, st));
    // the rows are read on `st`: the next poll (held rows) waits for that before it releases them, and a row that is not held
    // could be reused by a new game -- the handle's next steps then wait for the encode on the device
    if (!sp->enc_ev) HIPOK(hipEventCreateWithFlags(&sp->enc_ev, hipEventDisableTiming));
    HIPOK(hipEventRecord(sp->enc_ev, st));
    sp->enc_pending = true;
    if (!all_held) HIPOK(hipStreamWaitEvent(sp->stream, sp->enc_ev, 0));
    return 0;
}

int sc_selfplay_write_trace_json(sc_selfplay* sp, int game, const char* path) {
    TraceRow r;
    TRY(sp_read_trace(sp, game, TR_ALL, r));
    const uint16_t* line = nullptr;
    const int len = sp_opening(sp, game, &line);
    const char* fen = sp_opening_fen(sp, game);
    if (!path) return fail("bad argument");
    // a game that started from an opening line: a third key, "opening", behind the reference's two; from a base: "fen" in front of it
    return write_text_file(path, sctrace::trace_to_json(r.info.n_steps, r.info.has_outcome, r.info.termination, r.info.winner, r.move.data(), r.q.data(),
                                                        r.child_off.data(), r.cmove.data(), r.cn.data(), r.cq.data(), r.cu.data(), line, len, fen), false);
}

// Finished games as PGN: moves = opening line + played moves, rendered by one sc_moves_to_san_device_from call for the batch
int sc_selfplay_write_pgn(sc_selfplay* sp, int n, const int32_t* games, const char* path, int append, const char* white, const char* black,
                          const char* event) {
    if (!sp || n < 0 || (n > 0 && !games) || !path) return fail("bad argument");
    std::vector<sc_trace_info> info((size_t)std::max(n, 1));
    std::vector<uint16_t> moves;
    std::vector<uint32_t> off(1, 0);
    std::vector<int32_t> base_idx((size_t)std::max(n, 1), -1);
    std::vector<const char*> fens;
    int pending = 0;
    TraceRow r;
    for (int i = 0; i < n; i++) {   // every game must be ready (2 wins over 1, as sc_selfplay_encode_traces): nothing is written otherwise
        const int rc = sp_read_trace(sp, games[i], TR_MOVE, r);
        if (rc < 0 || rc == 2) return rc;
        pending |= rc;
        if (rc) continue;
        info[(size_t)i] = r.info;
        const uint16_t* line = nullptr;
        const int len = sp_opening(sp, games[i], &line);
        moves.insert(moves.end(), line, line + len);
        moves.insert(moves.end(), r.move.begin(), r.move.begin() + r.info.n_steps);
        off.push_back((uint32_t)moves.size());
        if (const char* fen = sp_opening_fen(sp, games[i])) {
            base_idx[(size_t)i] = (int32_t)fens.size();
            fens.push_back(fen);
        }
    }
    if (pending) return fail("game not finished", 1);
    const uint32_t P = off.back();
    std::vector<uint64_t> tok((size_t)P + 1);
    std::vector<int32_t> status((size_t)std::max(n, 1), 0);
    if (n > 0) {
        struct Bases {
            sc_positions* h = nullptr;
            ~Bases() { sc_positions_destroy(h); }
        } bases;
        if (!fens.empty()) TRY(sc_positions_from_fen(sp->device, (int)fens.size(), fens.data(), &bases.h, nullptr));
        ScopedDev<uint64_t> d_tok;
        ScopedDev<int32_t> d_status;
        HIPOK(d_tok.alloc(P));
        HIPOK(d_status.alloc((size_t)n));
        moves.push_back(0);   // (never an empty array)
        // on the NULL stream, like the copies of sc_selfplay_get_trace: held rows are written while the handle's stream works on
        TRY(sc_moves_to_san_device_from(sp->device, n, bases.h, base_idx.data(), moves.data(), off.data(), nullptr, d_tok.p, d_status.p));
        HIPOK(hipStreamSynchronize(nullptr));
        if (P) HIPOK(hipMemcpy(tok.data(), d_tok.p, (size_t)P * 8, hipMemcpyDeviceToHost));
        HIPOK(hipMemcpy(status.data(), d_status.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    std::string text;
    for (int i = 0; i < n; i++) {
        const sc_trace_info& t = info[(size_t)i];
        if (status[(size_t)i]) return fail("write_pgn: game " + std::to_string(games[i]) + ": move " + std::to_string(-status[(size_t)i] - 1) + " is not legal");
        // the White of game k is player k & 1 (sc_selfplay_set_match); against an outside opponent `white` names the engine
        // (sc_selfplay_set_external: colours = external - 1)
        const bool swapped = sp->external ? sp->external == 3 || (sp->external == 2 && (games[i] & 1)) : sp->p.match_colours && (games[i] & 1);
        const char* result = !t.has_outcome ? "*" : t.winner == 1 ? "1-0" : t.winner == 0 ? "0-1" : "1/2-1/2";
        text += pgn_tag("Event", event ? event : "?");
        text += pgn_tag("Round", std::to_string(t.game_id));
        text += pgn_tag("White", (swapped ? black : white) ? (swapped ? black : white) : "?");
        text += pgn_tag("Black", (swapped ? white : black) ? (swapped ? white : black) : "?");
        text += pgn_tag("Result", result);
        if (t.has_outcome) text += pgn_tag("Termination", sctrace::TERMINATION_NAMES[t.termination >= 0 && t.termination <= 10 ? t.termination : 0]);
        int fullmove = 1, black_first = 0;
        if (base_idx[(size_t)i] >= 0) {
            const char* fen = fens[(size_t)base_idx[(size_t)i]];
            sc_fen_fields ff;
            TRY(sc_fen_parse(fen, strlen(fen), &ff));
            fullmove = ff.fullmove;
            black_first = ff.turn == 0;
            text += pgn_tag("SetUp", "1");
            text += pgn_tag("FEN", fen);
        }
        const uint64_t* tk = tok.data() + off[(size_t)i];
        const uint32_t nt = off[(size_t)i + 1] - off[(size_t)i];
        std::string mt(scsan::san_format(tk, nt, (unsigned)fullmove, black_first != 0, result, nullptr, 0) + 1, '\0');
        scsan::san_format(tk, nt, (unsigned)fullmove, black_first != 0, result, &mt[0], mt.size());
        mt.pop_back();
        text += "\n" + pgn_wrap(mt) + "\n";
    }
    return write_text_file(path, text, append != 0);
}

int sc_selfplay_get_tree(sc_selfplay* sp, int slot, int cap, int32_t* n, float* q, float* uct, float* prior, uint16_t* move,
                         int32_t* first_child, int32_t* n_child) {
    if (!sp || slot < 0 || slot >= sp->p.n_slots) return fail("bad argument");
    const sc::SpParams& p = sp->p;
    sc::GameCtl c;
    TRY(sp_read_ctl(sp, slot, &c));
    int nn = std::min(c.n_nodes, cap);
    size_t nb = (size_t)slot * p.node_cap;
    if (nn > 0) {
        if (n) HIPOK(hipMemcpy(n, p.N + nb, (size_t)nn * 4, hipMemcpyDeviceToHost));
        if (q) HIPOK(hipMemcpy(q, p.W + nb, (size_t)nn * 4, hipMemcpyDeviceToHost));
        if (uct) HIPOK(hipMemcpy(uct, p.U + nb, (size_t)nn * 4, hipMemcpyDeviceToHost));
        if (prior) HIPOK(hipMemcpy(prior, p.P + nb, (size_t)nn * 4, hipMemcpyDeviceToHost));
        if (move) HIPOK(hipMemcpy(move, p.MV + nb, (size_t)nn * 2, hipMemcpyDeviceToHost));
        if (first_child || n_child) {
            std::vector<sc::NodeHdr> t((size_t)nn);
            HIPOK(hipMemcpy(t.data(), p.H + nb, (size_t)nn * sizeof(sc::NodeHdr), hipMemcpyDeviceToHost));
            for (int i = 0; i < nn; i++) {
                if (first_child) first_child[i] = t[(size_t)i].fc;
                if (n_child) n_child[i] = t[(size_t)i].nc;
            }
        }
    }
    return c.n_nodes;
}

int sc_selfplay_get_slot(sc_selfplay* sp, int slot, int32_t* ply, int32_t* sim, int32_t* status, uint64_t* game_id,
                         int32_t* last_path, int32_t* last_path_len) {
    if (!sp || slot < 0 || slot >= sp->p.n_slots) return fail("bad argument");
    sc::GameCtl c;
    TRY(sp_read_ctl(sp, slot, &c));
    if (ply) *ply = c.ply;
    if (sim) *sim = c.sim;
    if (status) *status = c.status;
    if (game_id) *game_id = c.game_id;
    if (last_path_len) *last_path_len = c.path_len;
    if (last_path && c.path_len > 0)
        HIPOK(hipMemcpy(last_path, sp->p.path + (size_t)slot * sp->p.max_depth, (size_t)std::min(c.path_len, 1024) * 4,
                        hipMemcpyDeviceToHost));
    return 0;
}

int sc_selfplay_set_noise(sc_selfplay* sp, int slot, const float* noise, int n) {
    if (!sp || slot < 0 || slot >= sp->p.n_slots || n < 0 || n > 224) return fail("bad argument");
    TRY(sp_quiesce(sp, false));
    HIPOK(hipMemcpy(sp->p.noise + (size_t)slot * 224, noise, (size_t)n * 4, hipMemcpyHostToDevice));
    return 0;
}
int sc_selfplay_get_noise(sc_selfplay* sp, int slot, float* noise, int cap) {
    if (!sp || slot < 0 || slot >= sp->p.n_slots) return fail("bad argument");
    TRY(sp_quiesce(sp, false));
    HIPOK(hipMemcpy(noise, sp->p.noise + (size_t)slot * 224, (size_t)std::min(cap, 224) * 4, hipMemcpyDeviceToHost));
    return 0;
}

int sc_selfplay_set_position(sc_selfplay* sp, int slot, const uint16_t* moves, int n_moves) {
    return sc_selfplay_set_position_from(sp, slot, nullptr, 0, moves, n_moves);
}

int sc_selfplay_set_position_from(sc_selfplay* sp, int slot, const sc_positions* bases, int i, const uint16_t* moves, int n_moves) {
    if (!sp || slot < 0 || slot >= sp->p.n_slots || n_moves < 0 || n_moves > 590) return fail("bad argument");
    const sc::Position* d_base = nullptr;
    if (bases) {
        TRY(positions_bases(bases, &i, 1, sp->device, true, "sc_selfplay_set_position_from", &d_base));
        if (i < 0) return fail("sc_selfplay_set_position_from: bad base index");
        d_base += i;
    }
    sc::GameCtl c;
    TRY(sp_read_ctl(sp, slot, &c));
    if (c.status == sc::ST_PENDING) return fail("slot is waiting for a trace-ring row: no game to reposition");
    ScopedDev<uint16_t> d_moves;
    HIPOK(d_moves.alloc((size_t)n_moves));
    if (n_moves) HIPOK(hipMemcpy(d_moves.p, moves, (size_t)n_moves * 2, hipMemcpyHostToDevice));
    scl::set_position(sp->p, slot, d_moves.p, n_moves, sp->stream, d_base);
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(sp->stream));
    return 0;
}

// Board.fen() of the slot's current position: the record is the last of the slot's chain; a lane of k_fen_ep_legal decides whether
// the ep square is printed, the text is formatted here
int sc_selfplay_get_fen(sc_selfplay* sp, int slot, char* buf, int cap) {
    if (!sp || slot < 0 || slot >= sp->p.n_slots || cap < 0 || (cap > 0 && !buf)) return fail("bad argument");
    sc::GameCtl c;
    TRY(sp_read_ctl(sp, slot, &c));
    if (c.status != sc::ST_ACTIVE && c.status != sc::ST_FINISHED) return fail("sc_selfplay_get_fen: the slot holds no game");
    if (c.ply < 0 || c.ply >= sp->p.hist_cap) return fail("sc_selfplay_get_fen: the slot's ply is outside its chain");
    const sc::Position* d_rec = sp->p.hist + (size_t)slot * sp->p.hist_cap + c.ply;
    ScopedDev<int32_t> d_epl;
    HIPOK(d_epl.alloc(1));
    scl::fen_ep_legal(1, d_rec, d_epl.p, sp->stream);
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(sp->stream));
    sc::Position rec;
    int32_t epl = 0;
    HIPOK(hipMemcpy(&rec, d_rec, sizeof rec, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(&epl, d_epl.p, 4, hipMemcpyDeviceToHost));
    return copy_text(position_fen(rec, epl != 0), buf, cap);
}

// One search from a given position: the body of NNPlayer::bestmove (src/play.rs:241-252) / chess_play_mcts
// (src/lib.rs:233-247) as a single call; see include/sc_engine.h
int sc_search(sc_engine* e, const uint16_t* moves, int n_moves, int rollout, float cpuct, int with_noise, uint64_t seed,
              int cap, uint16_t* child_move, int32_t* child_n, float* child_q, float* child_prior, float* root_q) {
    return sc_search_from(e, nullptr, 0, moves, n_moves, rollout, cpuct, with_noise, seed, cap, child_move, child_n, child_q, child_prior, root_q);
}

int sc_search_from(sc_engine* e, const sc_positions* bases, int base_i, const uint16_t* moves, int n_moves, int rollout, float cpuct,
                   int with_noise, uint64_t seed, int cap, uint16_t* child_move, int32_t* child_n, float* child_q, float* child_prior,
                   float* root_q) {
    if (!e || rollout < 1 || rollout >= 60000 || cap < 0) return fail("bad argument");
    // one cached handle per engine, rebuilt only when a call asks for more simulations than its node pools hold; every call starts
    // from a fresh one-node tree (sc_selfplay_set_position) with its own options and seed, so the result is that of a new handle
    int rc = 0;
    if (e->search_sp && (rollout + 1 > e->search_rollout_cap || e->search_sp->poisoned)) {
        sc_selfplay_destroy(e->search_sp);
        e->search_sp = nullptr;
    }
    if (!e->search_sp) {
        sc_selfplay_config c{};
        c.n_slots = 1;
        c.n_games = 1;
        c.rollout_num = std::max(rollout + 1, 512);   // sizes the node pool; more than any call runs, so no ply transition happens
        c.num_steps = 4000;
        c.cpuct = cpuct;
        c.epsilon = 0.15f;         // mcts::mcts(.., 0.15, noise) at both call sites
        c.with_noise = with_noise ? 1 : 0;
        c.outcome_gate = 1 << 30;
        c.evaluator = SC_EVAL_NET;
        c.seed = seed;
        rc = sc_selfplay_create(e, e->device, &c, &e->search_sp);
        if (rc) {
            e->search_sp = nullptr;
            return rc;
        }
        e->search_rollout_cap = c.rollout_num;
    }
    sc_selfplay* sp = e->search_sp;
    HIPOK(hipSetDevice(e->device));
    HIPOK(hipStreamSynchronize(sp->stream));
    sp->p.seed = seed;
    sp->cfg.seed = seed;
    rc = sc_selfplay_set_search(sp, cpuct, 0.15f, with_noise);
    {   // an earlier call's error flags are not this call's
        const int32_t zero = 0;
        HIPOK(hipMemcpy(reinterpret_cast<char*>(sp->p.cnt) + offsetof(sc::Counters, err), &zero, 4, hipMemcpyHostToDevice));
    }
    if (rc) return rc;
    rc = sc_selfplay_set_position_from(sp, 0, bases, base_i, moves, n_moves);
    if (!rc) rc = sc_selfplay_enqueue_sims(sp, rollout);
    int n_children = 0;
    if (!rc) {
        std::vector<int32_t> n(1 + 224), fc(1 + 224), nc(1 + 224);
        std::vector<float> q(1 + 224), pr(1 + 224);
        std::vector<uint16_t> mv(1 + 224);
        int nn = sc_selfplay_get_tree(sp, 0, 1 + 224, n.data(), q.data(), nullptr, pr.data(), mv.data(), fc.data(), nc.data());
        if (nn < 0) {
            rc = nn;
        } else {
            sc_selfplay_stats st{};
            rc = sc_selfplay_get_stats(sp, &st);
            if (!rc && st.error_flags) rc = fail("search error flags set (non-finite PUCT value or pool overflow)", -4);
            if (root_q) *root_q = nn > 0 ? q[0] : 0.f;
            n_children = nn > 0 && fc[0] == 1 ? nc[0] : 0;   // the root's children are nodes 1..nc
            for (int i = 0; i < n_children && i < cap; i++) {
                if (child_move) child_move[i] = mv[(size_t)1 + i];
                if (child_n) child_n[i] = n[(size_t)1 + i];
                if (child_q) child_q[i] = q[(size_t)1 + i];
                if (child_prior) child_prior[i] = pr[(size_t)1 + i];
            }
        }
    }
    return rc ? rc : n_children;
}

}  // extern "C"
