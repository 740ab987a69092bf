// sc-play -- batched evaluation matches on MI355X with the flags of the reference's `play` binary
// (reference src/play.rs:36-84 Args, :318-343 play_loop, :440-472 main; driven by scripts/leader-board:4-14):
//
//     sc-play --white-device cuda --white-checkpoint new.scw --black-device cuda --black-checkpoint old.scw \
//             -o "replay/w_{}.json" --rollout=100 --temperature 0 --temperature-switch 0 --cpuct 1.5 --games 100
//
// One process plays `--games` games of the pairing concurrently on one GPU (the reference plays one game per process
// under GNU parallel); "{}" in -o is replaced by the 1-based game number.  Every game is the reference loop: the two
// players alternate by ply on one shared tree cursor, no Dirichlet noise, temperature 1 below --temperature-switch,
// at temperature 0 a random child among the most visited, outcome(claim_draw=True) after every ply, at most 200 plies,
// the outcome (or null) stored in the trace.  Stockfish opponents (--black-type stockfish) are out of scope.
// Extra flags (no reference counterpart): --games, --seed, --blocks / --channels / --white-seed / --black-seed (random
// networks when no checkpoint is given).
// --concurrency C plays the games on C recycled slots (sc_selfplay_set_match): a finished game's slot goes on with the next game.
// --swap also plays --games games with the colours exchanged, in the same handle (scripts/leader-board:44-54 runs `play` twice):
// their traces go to --swap-output (the leader-board's b_ prefix), numbered 1..games like the first set.  Without these flags
// all games run in lockstep on --games slots, as before.
// --openings FILE starts game k from line k of FILE (sc_selfplay_set_openings; with --swap both games of a pair from the same line,
// each network White once).  One line per opening: UCI moves separated by blanks; `#` starts a comment (a line that holds nothing
// but a comment is skipped); an empty line is the start position; a line whose first word is `fen` is
// `fen <the 4 or 6 fields> [moves m1 m2 ...]` and starts from that position (sc_selfplay_set_openings_from).  The games then run on
// recycled slots (--concurrency, default one slot per game).
// --pgn FILE also writes the whole match as one PGN file (sc_selfplay_write_pgn: SAN rendered on the GPU), with --swap both colour
// assignments in it; White and Black are named after their checkpoint files (net-seed<N> for a random network).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/sc_engine.h"

struct Args {
    std::string white_device, black_device = "<not-specified>", black_type = "stockfish";
    std::string black_checkpoint = "<not-specified>", white_checkpoint = "<not-specified>", output = "01.json", swap_output, openings, pgn;
    int rollout = 60, temperature_switch = 0, games = 1, blocks = 10, channels = 256, concurrency = 0;
    bool swap = false, has_pgn = false;
    float temperature = 0.0f, cpuct = 0.0f;
    unsigned long long seed = 0xC0FFEEULL, white_seed = 1, black_seed = 2;
};

static void usage() {
    fprintf(stderr,
            "usage: sc-play --white-device cuda -w|--white-checkpoint W.scw [--black-device cuda] [--black-type nn]\n"
            "               [--black-checkpoint B.scw] [-r|--rollout 60] [--temperature 0] [--temperature-switch 0] [--cpuct 0]\n"
            "               [-o|--output 01.json] [--games 1] [--seed S] [--blocks 10] [--channels 256] [--white-seed 1] [--black-seed 2]\n"
            "               [--concurrency SLOTS] [--swap --swap-output b_01.json] [--openings FILE] [--pgn FILE]\n");
}

static bool parse(int argc, char** argv, Args& a) {
    for (int i = 1; i < argc; i++) {
        std::string k = argv[i], v;
        size_t eq = k.find('=');
        bool has = false;
        if (k.rfind("--", 0) == 0 && eq != std::string::npos) {   // --rollout=100 form (scripts/leader-board:46)
            v = k.substr(eq + 1);
            k = k.substr(0, eq);
            has = true;
        }
        auto val = [&]() -> const char* {
            if (has) return v.c_str();
            if (i + 1 >= argc) {
                fprintf(stderr, "missing value for %s\n", k.c_str());
                exit(2);
            }
            return argv[++i];
        };
        if (k == "--white-device") a.white_device = val();
        else if (k == "--black-device") a.black_device = val();
        else if (k == "--black-type") a.black_type = val();
        else if (k == "--stockfish-bin" || k == "--stockfish-level") (void)val();
        else if (k == "--black-checkpoint") a.black_checkpoint = val();
        else if (k == "-w" || k == "--white-checkpoint") a.white_checkpoint = val();
        else if (k == "-r" || k == "--rollout") a.rollout = atoi(val());
        else if (k == "--temperature") a.temperature = (float)atof(val());
        else if (k == "--temperature-switch") a.temperature_switch = atoi(val());
        else if (k == "--cpuct") a.cpuct = (float)atof(val());
        else if (k == "-o" || k == "--output") a.output = val();
        else if (k == "--games") a.games = atoi(val());
        else if (k == "--concurrency") a.concurrency = atoi(val());
        else if (k == "--swap" && !has) a.swap = true;
        else if (k == "--swap-output") a.swap_output = val();
        else if (k == "--openings") a.openings = val();
        else if (k == "--pgn") { a.pgn = val(); a.has_pgn = true; }
        else if (k == "--seed") a.seed = strtoull(val(), nullptr, 0);
        else if (k == "--blocks") a.blocks = atoi(val());
        else if (k == "--channels") a.channels = atoi(val());
        else if (k == "--white-seed") a.white_seed = strtoull(val(), nullptr, 0);
        else if (k == "--black-seed") a.black_seed = strtoull(val(), nullptr, 0);
        else if (k == "-h" || k == "--help") { usage(); exit(0); }
        else { fprintf(stderr, "unknown argument %s\n", k.c_str()); usage(); return false; }
    }
    return true;
}

// UCI text -> move (from | to << 6 | promo << 12), 0xffff if it is none
static unsigned parse_uci(const std::string& t) {
    if (t.size() < 4 || t.size() > 5) return 0xffff;
    for (int i = 0; i < 4; i += 2)
        if (t[i] < 'a' || t[i] > 'h' || t[i + 1] < '1' || t[i + 1] > '8') return 0xffff;
    unsigned promo = 0;
    if (t.size() == 5) {
        const char* at = strchr("nbrq", t[4]);
        if (!at || !t[4]) return 0xffff;
        promo = 2u + (unsigned)(at - "nbrq");
    }
    return (unsigned)((t[1] - '1') * 8 + (t[0] - 'a')) | (unsigned)((t[3] - '1') * 8 + (t[2] - 'a')) << 6 | promo << 12;
}

// the opening file: moves and offsets as sc_selfplay_set_openings takes them, and the file's line number of every opening.  A line
// whose first word is `fen` is `fen <the 4 or 6 fields> [moves m1 m2 ...]` (the UCI `position` convention): fens holds its FEN text,
// "" for every other line; the text's syntax is checked here (sc_fen_parse needs no GPU)
static bool read_openings(const std::string& path, std::vector<uint16_t>& moves, std::vector<uint32_t>& off, std::vector<int>& line_no,
                          std::vector<std::string>& fens) {
    std::ifstream f(path);
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path.c_str());
        return false;
    }
    off.assign(1, 0);
    std::string raw;
    for (int no = 1; std::getline(f, raw); no++) {
        const size_t hash = raw.find('#');
        std::istringstream text(raw.substr(0, hash));
        std::string tok, fen;
        size_t n = 0;
        bool in_fen = false, first = true;
        while (text >> tok) {
            if (first && tok == "fen") {
                in_fen = true;
                first = false;
                continue;
            }
            first = false;
            if (in_fen) {
                if (tok == "moves") in_fen = false;
                else fen += (fen.empty() ? "" : " ") + tok;
                continue;
            }
            const unsigned m = parse_uci(tok);
            if (m == 0xffff) {
                fprintf(stderr, "%s:%d: '%s' is not a UCI move\n", path.c_str(), no, tok.c_str());
                return false;
            }
            moves.push_back((uint16_t)m);
            n++;
        }
        if (n == 0 && fen.empty() && hash != std::string::npos) continue;   // a comment line
        if (!fen.empty()) {
            sc_fen_fields ff;
            if (sc_fen_parse(fen.data(), fen.size(), &ff)) {
                fprintf(stderr, "%s:%d: '%s': %s\n", path.c_str(), no, fen.c_str(), sc_last_error());
                return false;
            }
        }
        off.push_back((uint32_t)moves.size());
        line_no.push_back(no);
        fens.push_back(fen);
    }
    if (line_no.empty()) {
        fprintf(stderr, "%s: no opening lines\n", path.c_str());
        return false;
    }
    return true;
}

// a player's name in the PGN: its checkpoint's file name, or net-seed<N> for a random network
static std::string player_name(const std::string& checkpoint, unsigned long long seed) {
    if (checkpoint == "<not-specified>") return "net-seed" + std::to_string(seed);
    const size_t slash = checkpoint.find_last_of('/');
    return slash == std::string::npos ? checkpoint : checkpoint.substr(slash + 1);
}

static std::string out_name(const Args& a, const std::string& pattern, int game_number) {
    std::string t = pattern;
    size_t p = t.find("{}");
    if (p != std::string::npos) return t.substr(0, p) + std::to_string(game_number) + t.substr(p + 2);
    if (a.games == 1) return t;
    size_t dot = t.rfind('.');
    if (dot == std::string::npos) return t + std::to_string(game_number);
    return t.substr(0, dot) + "_" + std::to_string(game_number) + t.substr(dot);
}

int main(int argc, char** argv) {
    setenv("HIP_FORCE_DEV_KERNARG", "1", 0);   // kernel arguments in device memory; before any HIP call
    Args a;
    if (!parse(argc, argv, a)) return 2;
    if (a.white_device.empty()) {   // clap: required argument
        fprintf(stderr, "--white-device is required\n");
        return 2;
    }
    if (a.black_checkpoint != "<not-specified>") a.black_type = "nn";   // play.rs:405-408
    if (a.black_type != "nn" && a.black_type != "NN") {
        fprintf(stderr, "black-type '%s' is not supported: only network-vs-network matches are built (Stockfish/UCI is out of scope)\n",
                a.black_type.c_str());
        return 2;
    }
    if (a.white_device != "cuda") {
        fprintf(stderr, "device '%s' is not supported: this launcher has no CPU path\n", a.white_device.c_str());
        return 2;
    }
    if (a.games < 1 || a.rollout < 1) {
        fprintf(stderr, "--games and --rollout must be positive\n");
        return 2;
    }
    const bool recycle = a.swap || a.concurrency != 0 || !a.openings.empty();
    std::vector<uint16_t> op_moves;
    std::vector<uint32_t> op_off;
    std::vector<int> op_line_no;
    std::vector<std::string> op_fens;
    if (!a.openings.empty() && !read_openings(a.openings, op_moves, op_off, op_line_no, op_fens)) return 2;
    if (a.swap == a.swap_output.empty()) {
        fprintf(stderr, "--swap and --swap-output go together\n");
        return 2;
    }
    if (a.has_pgn && (a.pgn.empty() || a.pgn[0] == '-')) {
        fprintf(stderr, "--pgn needs a file name\n");
        usage();
        return 2;
    }
    if (recycle && a.concurrency < 0) {
        fprintf(stderr, "--concurrency must be positive\n");
        return 2;
    }
    if (sc_device_count() <= 0) {
        fprintf(stderr, "no MI355X visible\n");
        return 1;
    }
    sc_engine *w = nullptr, *b = nullptr;
    sc_net_config wc{a.blocks, a.channels, a.white_seed}, bc{a.blocks, a.channels, a.black_seed};
    if (sc_engine_create(&wc, a.white_checkpoint == "<not-specified>" ? nullptr : a.white_checkpoint.c_str(), 0, &w) ||
        sc_engine_create(&bc, a.black_checkpoint == "<not-specified>" ? nullptr : a.black_checkpoint.c_str(), 0, &b)) {
        fprintf(stderr, "%s\n", sc_last_error());
        return 1;
    }
    printf("Players loaded.\n");   // play.rs:455
    sc_selfplay_config c{};
    const int total = a.swap ? 2 * a.games : a.games;
    c.n_games = total;
    c.n_slots = recycle ? (a.concurrency > 0 && a.concurrency < total ? a.concurrency : total) : a.games;
    c.rollout_num = a.rollout;
    c.num_steps = 200;             // play.rs:325
    c.cpuct = a.cpuct;
    c.temperature = a.temperature;
    c.temperature_switch = a.temperature_switch;
    c.epsilon = 0.15f;
    c.with_noise = 0;              // play.rs:250
    c.outcome_gate = -1;           // play.rs:335: after every ply
    c.evaluator = SC_EVAL_NET;
    c.seed = a.seed;
    c.tie_random = 1;              // play.rs:268-277
    sc_selfplay* sp = nullptr;
    int rc = sc_selfplay_create(w, 0, &c, &sp);
    if (!rc) rc = recycle ? sc_selfplay_set_match(sp, w, b, 0, 0, a.swap ? 1 : 0) : sc_selfplay_set_players(sp, w, b, 0, 0);
    if (!rc && !a.openings.empty()) {
        std::vector<int32_t> status(op_line_no.size(), 0);
        op_moves.push_back(0);   // (never an empty array)
        // lines that start from a FEN: one validated set of their positions, a base index per line
        std::vector<const char*> texts;
        std::vector<int32_t> base_idx(op_line_no.size(), -1);
        for (size_t i = 0; i < op_fens.size(); i++)
            if (!op_fens[i].empty()) {
                base_idx[i] = (int32_t)texts.size();
                texts.push_back(op_fens[i].c_str());
            }
        sc_positions* bases = nullptr;
        if (!texts.empty()) rc = sc_positions_from_fen(0, (int)texts.size(), texts.data(), &bases, nullptr);
        if (!rc) rc = sc_selfplay_set_openings_from(sp, (int)op_line_no.size(), bases, base_idx.data(), op_moves.data(), op_off.data(), status.data());
        for (size_t i = 0; i < status.size(); i++)
            if (status[i]) fprintf(stderr, "%s:%d: opening refused, status %d\n", a.openings.c_str(), op_line_no[i], status[i]);
        sc_positions_destroy(bases);   // (the handle keeps its own records of the lines)
    }
    if (!rc) rc = sc_selfplay_run(sp, 0);
    if (rc) {
        fprintf(stderr, "%s\n", sc_last_error());
        return 1;
    }
    // [0]: the games with --white-checkpoint's network as White, [1] (--swap): as Black; White won / Black won / draw / no outcome
    long long res[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    std::vector<int32_t> finished;
    std::vector<std::string> paths;
    for (int g = 0; g < total; g++) {
        sc_trace_info info{};
        if (sc_selfplay_get_trace(sp, g, &info, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)) continue;
        finished.push_back(g);
        const int set = a.swap ? (int)(info.game_id & 1) : 0;
        res[set][!info.has_outcome ? 3 : info.winner == 1 ? 0 : info.winner == 0 ? 1 : 2]++;
        const int number = (int)(a.swap ? info.game_id / 2 : info.game_id) + 1;
        paths.push_back(out_name(a, set ? a.swap_output : a.output, number));
    }
    // every trace file in one call: the text is formatted on the device (sc_selfplay_write_traces_json)
    std::vector<const char*> cpaths;
    for (const std::string& p : paths) cpaths.push_back(p.c_str());
    if (sc_selfplay_write_traces_json(sp, (int)finished.size(), finished.data(), cpaths.data())) {
        fprintf(stderr, "%s\n", sc_last_error());
        rc = 1;
    }
    if (a.has_pgn && sc_selfplay_write_pgn(sp, (int)finished.size(), finished.data(), a.pgn.c_str(), 0,
                                           player_name(a.white_checkpoint, a.white_seed).c_str(),
                                           player_name(a.black_checkpoint, a.black_seed).c_str(), "sc-play match")) {
        fprintf(stderr, "%s\n", sc_last_error());
        rc = 1;
    }
    if (!recycle) {
        // Total/WhiteWin/BlackWin is the input format of scripts/elo.py
        printf("games %d white-wins %lld black-wins %lld draws %lld unfinished %lld   (elo.py input: %d/%lld/%lld)\n", a.games, res[0][0], res[0][1],
               res[0][2], res[0][3], a.games, res[0][0], res[0][1]);
    } else {
        // the device's tally, which must agree with the traces just written; the elo.py triple is Total / wins of the --white-checkpoint
        // network / wins of the --black-checkpoint network over both colour assignments
        int64_t tally[8] = {0};
        if (sc_selfplay_match_tally(sp, tally)) {
            fprintf(stderr, "%s\n", sc_last_error());
            rc = 1;
        }
        for (int i = 0; i < 8; i++)
            if (tally[i] != res[i / 4][i % 4]) {
                fprintf(stderr, "match tally [%d] = %lld differs from the traces' %lld\n", i, (long long)tally[i], res[i / 4][i % 4]);
                rc = 1;
            }
        printf("games %d slots %d as-white: white-wins %lld black-wins %lld draws %lld unfinished %lld", total, c.n_slots, (long long)tally[0],
               (long long)tally[1], (long long)tally[2], (long long)tally[3]);
        if (a.swap)
            printf("  as-black: white-wins %lld black-wins %lld draws %lld unfinished %lld", (long long)tally[4], (long long)tally[5],
                   (long long)tally[6], (long long)tally[7]);
        printf("   (elo.py input: %d/%lld/%lld)\n", total, (long long)(tally[0] + tally[5]), (long long)(tally[1] + tally[4]));
    }
    sc_selfplay_destroy(sp);
    sc_engine_destroy(w);
    sc_engine_destroy(b);
    return rc;
}
