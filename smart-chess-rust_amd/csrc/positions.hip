// positions.hip -- host side of libsc_engine.so: positions given as FEN (sc_fen_parse, sc_positions_*; include/sc_engine.h).
// The text is read on the host (fen_text.cpp: no rules code), the fields become validated records on the device
// (fen_kernels.hip), and the set keeps a host copy of records, status and the ep bit of Board.fen(), so that its accessors and the
// checks of the entry points that take bases need no device work.
#include <string.h>

#include "fen_text.hpp"
#include "host_common.hpp"

std::string position_fen(const sc::Position& p, bool ep_legal) {
    sc_fen_fields f{};
    for (int t = 0; t < 6; t++) f.pcs[t] = p.pcs[t];
    f.occ[0] = p.occ[0];
    f.occ[1] = p.occ[1];
    f.turn = p.turn;
    f.castling = p.castling;
    f.ep = p.ep;
    f.halfmove = p.halfmove;
    f.fullmove = p.fullmove;
    char buf[128];
    scfen::fen_format(&f, ep_legal, buf, (int)sizeof buf);
    return buf;
}

int copy_text(const std::string& s, char* buf, int cap) {
    if (cap > 0) {
        const size_t k = std::min(s.size(), (size_t)cap - 1);
        memcpy(buf, s.data(), k);
        buf[k] = 0;
    }
    return (int)s.size();
}

int positions_bases(const sc_positions* bases, const int32_t* idx, int n, int dev, bool for_search, const char* who, const sc::Position** d_rec) {
    *d_rec = nullptr;
    if (!bases || !idx) return 0;
    if (bases->device != dev)
        return fail(std::string(who) + ": the positions live on device " + std::to_string(bases->device) + ", the call runs on device " + std::to_string(dev));
    for (int k = 0; k < n; k++) {
        const int i = idx[k];
        if (i < 0) continue;
        if (i >= bases->n) return fail(std::string(who) + ": base index " + std::to_string(i) + " of " + std::to_string(bases->n) + " positions");
        const int st = bases->status[(size_t)i];
        if (st < 0) return fail(std::string(who) + ": position " + std::to_string(i) + " cannot be played (status " + std::to_string(st) + ")");
        if (st == 1 && for_search) return fail(std::string(who) + ": the game is over in position " + std::to_string(i) + " (status 1): nothing to search");
    }
    *d_rec = bases->d_rec;
    return 0;
}

extern "C" {

int sc_fen_parse(const char* text, size_t len, sc_fen_fields* out) {
    if (!out || (!text && len)) return fail("bad argument");
    const int rc = scfen::fen_parse(text, len, out);
    if (rc) {
        static const char* const names[] = {"", "board", "turn", "castling", "ep", "halfmove", "fullmove"};
        return fail(std::string("sc_fen_parse: bad ") + names[-rc] + " field", rc);
    }
    return 0;
}

int sc_positions_from_fen(int device_id, int n, const char* const* fens, sc_positions** out, int32_t* status) {
    if (out) *out = nullptr;
    TRY(use_device(nullptr, device_id));
    if (n < 0 || !out || (n > 0 && !fens)) return fail("bad argument");
    std::vector<sc_fen_fields> fields((size_t)std::max(n, 1));
    std::vector<int32_t> syntax((size_t)std::max(n, 1), 0);
    for (int i = 0; i < n; i++) {
        if (!fens[i]) {
            scfen::fen_startpos(&fields[(size_t)i]);
            continue;
        }
        const int rc = scfen::fen_parse(fens[i], strlen(fens[i]), &fields[(size_t)i]);
        if (rc) syntax[(size_t)i] = -(100 - rc);   // rc = -(field): -(100 + field)
    }
    ScopedDev<sc_fen_fields> d_fields;
    ScopedDev<int32_t> d_syntax, d_status, d_epl;
    ScopedDev<sc::Position> d_rec;
    HIPOK(d_fields.alloc((size_t)n));
    HIPOK(d_syntax.alloc((size_t)n));
    HIPOK(d_status.alloc((size_t)n));
    HIPOK(d_epl.alloc((size_t)n));
    HIPOK(d_rec.alloc((size_t)n));
    sc_positions* ps = new sc_positions();
    ps->device = device_id;
    ps->n = n;
    ps->rec.resize((size_t)n);
    ps->status.resize((size_t)n);
    ps->ep_legal.resize((size_t)n);
    struct Guard {
        sc_positions* p;
        ~Guard() { delete p; }
    } guard{ps};
    if (n) {
        HIPOK(hipMemcpy(d_fields.p, fields.data(), (size_t)n * sizeof(sc_fen_fields), hipMemcpyHostToDevice));
        HIPOK(hipMemcpy(d_syntax.p, syntax.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        scl::fen_positions(n, d_fields.p, d_syntax.p, d_rec.p, d_status.p, nullptr);
        scl::fen_ep_legal(n, d_rec.p, d_epl.p, nullptr);
        HIPOK(hipGetLastError());
        HIPOK(hipDeviceSynchronize());
        HIPOK(hipMemcpy(ps->rec.data(), d_rec.p, (size_t)n * sizeof(sc::Position), hipMemcpyDeviceToHost));
        HIPOK(hipMemcpy(ps->status.data(), d_status.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        HIPOK(hipMemcpy(ps->ep_legal.data(), d_epl.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    if (status) std::copy(ps->status.begin(), ps->status.end(), status);
    ps->d_rec = d_rec.p;
    d_rec.p = nullptr;
    guard.p = nullptr;
    *out = ps;
    return 0;
}

void sc_positions_destroy(sc_positions* ps) {
    if (!ps) return;
    if (ps->d_rec && hipSetDevice(ps->device) == hipSuccess) (void)hipFree(ps->d_rec);
    delete ps;
}

int sc_positions_count(const sc_positions* ps) { return ps ? ps->n : fail("null handle"); }

int sc_positions_status(const sc_positions* ps, int i) {
    if (!ps || i < 0 || i >= ps->n) return fail("bad argument", -1000);   // (-1 is a status)
    return ps->status[(size_t)i];
}

int sc_positions_fen(const sc_positions* ps, int i, char* buf, int cap) {
    if (!ps || i < 0 || i >= ps->n || cap < 0 || (cap > 0 && !buf)) return fail("bad argument");
    if (ps->status[(size_t)i] < 0) return fail("sc_positions_fen: position " + std::to_string(i) + " was refused (status " + std::to_string(ps->status[(size_t)i]) + ")");
    return copy_text(position_fen(ps->rec[(size_t)i], ps->ep_legal[(size_t)i] != 0), buf, cap);
}

}  // extern "C"
