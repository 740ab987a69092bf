"""Rate of writing trace files: the host writer (sc_trace_write_json, one call and one file per game) against the device writer
(sc_traces_format: csrc/trace_write_kernels.hip, all games in one call), on the 256-game trace set of tools/ratelib.py with
pseudo-random float32 Q and uct values, as tools/trace_read_rate.py writes them.  Prints one JSON line and appends it to
profiles/trace_write_rate_<date>.jsonl (--out).

  python tools/trace_write_rate.py [--reps 5] [--games N] [--out FILE]

--games N: the first N games only (the small form).  The texts of the two writers are compared equal before anything is timed.
rows:
  host          sc_trace_write_json per game, files written
  device        sc_traces_format with the sizes known (the emitting call alone: the counting pass runs in it again), text in memory
  device_files  the same, and every game's text written to its file
  call_ms       host wall time of the whole row; medians over --reps calls after one warm-up call (ratelib.Hip.timed)
  count_ms / emit_ms   HIP events around the two passes of the last device call (sc_traces_format_last_timing);
  emit_text_GB_per_s   the text's bytes over emit_ms, and hbm_frac, that rate against the 8 TB/s of the HBM"""
import argparse
import os
import tempfile

import numpy as np

from ratelib import Hip, common_args, emit, ptr, record, require_device, spread, trace_set  # sets the package path

import scamd  # noqa: E402
import scamd.traces  # noqa: E402

HBM_GB_PER_S = 8000.0


def make_traces(games):
    rng = np.random.default_rng(7)
    return [{"steps": [(s[0], float(rng.normal() * 5), [(c[0], c[1], float(rng.normal()), float(rng.random())) for c in s[1]]) for s in steps],
             "outcome": {"termination": "Checkmate", "winner": ("White", "Black")[g & 1]} if g % 3 else None} for g, steps in enumerate(games)]


def main():
    ap = argparse.ArgumentParser()
    common_args(ap, reps=5)
    ap.add_argument("--games", type=int, default=256, help="the first N games of the set")
    ap.add_argument("--out", default=None, help="result file (default profiles/trace_write_rate_<date>.jsonl)")
    args = ap.parse_args()
    L = require_device()
    eng = scamd.Engine(args.blocks, args.channels, seed=1)
    traces = make_traces(trace_set(eng)[:args.games])
    eng.close()
    hip = Hip(L)
    n = len(traces)
    with tempfile.TemporaryDirectory() as folder:
        paths = [os.path.join(folder, f"trace_{g:04d}.json") for g in range(n)]

        def host():
            for p, t in zip(paths, traces):
                scamd.write_trace_json(p, t)
            return 0

        host()
        want = [open(p, "rb").read() for p in paths]
        if scamd.traces.format(traces) != want:
            raise SystemExit("the device writer's texts differ from the host writer's")
        fmt_args, keep = scamd.traces.pack_traces(traces)
        off = np.zeros(n + 1, np.uint64)
        assert L.sc_traces_format(0, n, *fmt_args, None, 0, ptr(off)) == 0, L.sc_last_error().decode()
        n_bytes = int(off[n])
        text = np.zeros(max(n_bytes, 1), np.uint8)

        def device():
            return L.sc_traces_format(0, n, *fmt_args, ptr(text), n_bytes, ptr(off))

        def device_files():
            rc = device()
            for g, p in enumerate(paths):
                with open(p, "wb") as f:
                    f.write(text[int(off[g]):int(off[g + 1])].data)
            return rc

        rows = {}
        for name, fn in (("host", host), ("device", device), ("device_files", device_files)):
            c = spread(hip.timed(fn, args.reps)[0])
            rows[name] = {"call_ms": round(c[0], 2), "call_ms_min": round(c[1], 2), "call_ms_max": round(c[2], 2),
                          "text_MB_per_s": round(n_bytes / 1e6 / (c[0] * 1e-3), 1), "games_per_s": round(n / (c[0] * 1e-3), 1)}
            if name == "device":
                count_ms, emit_ms = scamd.traces.format_last_timing()
                gbps = n_bytes / 1e9 / (emit_ms * 1e-3)
                rows[name].update(count_ms=round(count_ms, 3), emit_ms=round(emit_ms, 3), emit_text_GB_per_s=round(gbps, 2),
                                  hbm_frac=round(gbps / HBM_GB_PER_S, 6))
        if [open(p, "rb").read() for p in paths] != want:
            raise SystemExit("device_files: the files differ from the host writer's")
        del keep
    hip.close()
    plies = sum(len(t["steps"]) for t in traces)
    emit([record("trace_write_rate", games=n, plies=plies, children=sum(len(s[2]) for t in traces for s in t["steps"]), text_bytes=n_bytes,
                 bytes_per_game=n_bytes // max(n, 1), reps=args.reps, rows=rows,
                 host_over_device=round(rows["host"]["call_ms"] / rows["device"]["call_ms"], 2))], args.out, "trace_write_rate")


if __name__ == "__main__":
    main()
