"""Rate of reading trace files into training tensors: the Python reader (json.loads, the list form, pack_steps, encode_steps_torch)
against the device reader (scamd.traces.read + encode_traces_torch: csrc/trace_kernels.hip), on the 256-game trace set of
tools/ratelib.py written to text with sc_trace_write_json.  Prints one JSON line and appends it to
profiles/trace_read_rate_<date>.jsonl (--out).

  python tools/trace_read_rate.py [--reps 5] [--out FILE]

rows, all from the same bytes to the same tensors (layout "reference", dist "legal"; checked equal with torch.equal):
  python        json.loads + validate_model.load_trace's comprehension + pack_steps + encode_steps_torch, text in memory
  device        traces.read + encode_traces_torch, text in memory
  device_files  the same from files on disk (open(..., "rb") of every file inside the timing)
  call_ms       host wall time of the whole call, the wait for its work included (both paths end with the host's copy of the
                status).  Medians over --reps calls after one warm-up call (ratelib.Hip.timed).
  parse_count_ms / parse_emit_ms   HIP events around the two parse passes of the last device read (sc_traces_last_timing)
  encode_device_ms                 HIP events around sc_traces_encode_device alone, on the parsed set
The Q and uct values of the written text are pseudo-random float32, so that a child takes the bytes it takes in a real trace."""
import argparse
import ctypes as C
import json
import os
import tempfile

import torch  # noqa: F401  (first: libsc_engine.so then binds to the HIP runtime torch loaded)
import numpy as np

from ratelib import Hip, common_args, emit, record, require_device, spread, trace_set  # sets the package path

import scamd  # noqa: E402
import scamd.traces  # noqa: E402

KEYS = ("boards", "meta", "dist_legal", "legal_idx", "n_legal", "outcome")


def write_texts(games, folder):
    rng = np.random.default_rng(7)
    paths = []
    for g, steps in enumerate(games):
        tr = {"steps": [(s[0], float(rng.normal() * 5), [(c[0], c[1], float(rng.normal()), float(rng.random())) for c in s[1]]) for s in steps],
              "outcome": {"termination": "Checkmate", "winner": ("White", "Black")[g & 1]} if g % 3 else None}
        paths.append(os.path.join(folder, f"trace_{g:04d}.json"))
        scamd.write_trace_json(paths[-1], tr)
    return paths


def python_path(texts):
    games, wins = [], []
    for t in texts:
        tr = json.loads(t)
        games.append([(s[0], [(c[0], int(c[1])) for c in s[2]]) for s in tr["steps"]])
        oc = tr.get("outcome")
        wins.append(0.0 if not oc or oc.get("winner") is None else 1.0 if oc["winner"] == "White" else -1.0)
    return scamd.encode_steps_torch(scamd.pack_steps(games), layout="reference", dist="legal", outcomes=wins)


def device_path(sources):
    t = scamd.traces.read(sources)
    try:
        return scamd.traces.encode_traces_torch(t.check(), layout="reference", dist="legal")
    finally:
        t.close()


def main():
    ap = argparse.ArgumentParser()
    common_args(ap, reps=5)
    ap.add_argument("--out", default=None, help="result file (default profiles/trace_read_rate_<date>.jsonl)")
    args = ap.parse_args()
    L = require_device()
    eng = scamd.Engine(args.blocks, args.channels, seed=1)
    games = trace_set(eng)
    eng.close()
    hip = Hip(L)
    with tempfile.TemporaryDirectory() as folder:
        paths = write_texts(games, folder)
        texts = [open(p, "rb").read() for p in paths]
        n_bytes, P = sum(len(t) for t in texts), sum(len(g) for g in games)
        want = python_path(texts)
        for name, src in (("device", texts), ("device_files", paths)):
            got = device_path(src)
            if got["status"].any() or want["status"].any() or not all(torch.equal(got[k], want[k]) for k in KEYS):
                raise SystemExit(f"{name}: the tensors differ from the Python reader's")
        def run(fn, arg):   # (Hip.timed takes a call that returns the entry point's code)
            fn(arg)
            return 0

        rows = {}
        for name, fn, arg in (("python", python_path, texts), ("device", device_path, texts), ("device_files", device_path, paths)):
            c = spread(hip.timed(lambda: run(fn, arg), args.reps)[0])
            rows[name] = {"call_ms": round(c[0], 2), "call_ms_min": round(c[1], 2), "call_ms_max": round(c[2], 2),
                          "text_MB_per_s": round(n_bytes / 1e6 / (c[0] * 1e-3), 1), "plies_per_s": round(P / (c[0] * 1e-3), 1)}
            if name == "device":
                a, b = C.c_float(0), C.c_float(0)
                L.sc_traces_last_timing(C.byref(a), C.byref(b))
                rows[name].update(parse_count_ms=round(a.value, 3), parse_emit_ms=round(b.value, 3),
                                  parse_text_GB_per_s=round(n_bytes / 1e9 / ((a.value + b.value) * 1e-3), 2))
        # the encoder alone on a parsed set, into buffers of the tool (HIP events on the tool's stream)
        t = scamd.traces.read(texts)
        out = [hip.alloc(P * 7168), hip.alloc(P * 28), None, hip.alloc(P * 224 * 4), hip.alloc(P * 448), hip.alloc(P * 4), hip.alloc(len(games) * 4)]
        dev_ms = hip.timed(lambda: L.sc_traces_encode_device(None, t.h, 0, len(games), 0, 0, hip.stream, *out), args.reps)[2]
        rows["device"]["encode_device_ms"] = round(spread(dev_ms)[0], 3)
        t.close()
    hip.close()
    emit([record("trace_read_rate", games=len(games), plies=P, text_bytes=n_bytes, bytes_per_game=n_bytes // len(games), reps=args.reps, rows=rows,
                 python_over_device=round(rows["python"]["call_ms"] / rows["device"]["call_ms"], 2))], args.out, "trace_read_rate")


if __name__ == "__main__":
    main()
