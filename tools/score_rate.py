"""Rate of scoring networks on device tensors (sc_score_positions in both dist forms, sc_compare_engines) on the 256-game trace
set of tools/encode_device_rate.py, next to (a) the forward pass alone on the same positions (sc_forward_device without the
log-probabilities: the floor) and (b) the route that exists without these entry points: sc_forward_batch with the
log-probabilities copied to the host and the float64 numpy formulas there.  Appends one JSON line to
profiles/score_rate_<date>.jsonl and prints it.

  python tools/score_rate.py [--reps 7] [--blocks 10] [--channels 128]

Every device figure is the median over --reps regions after one warm-up call, with the smallest and largest region next to it
(device_ms_min / _max): HIP events on the stream around the call (device_ms) and host wall time including the wait for the
stream (call_ms).  positions_per_s is P / device_ms in every row.  The scoring kernels' own time is NOT derived from these
(the difference of two calls is smaller than their spread): it comes from a kernel trace of this tool,

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/score_rate.py --forms dense --no-host-route --out /dev/null
  python tools/score_kernel_times.py DIR --label dense

one run per form (--forms dense | sparse | compare), so that a kernel name means one thing in a trace."""
import argparse
import ctypes as C
import datetime
import json
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smart-chess-rust_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import scamd  # noqa: E402
from encode_device_rate import trace_set  # noqa: E402



def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--forms", default="dense,sparse,compare", help="which calls to run (comma list of dense, sparse, compare)")
    ap.add_argument("--no-host-route", action="store_true", help="skip the sc_forward_batch + numpy baseline")
    ap.add_argument("--out", default=None, help="result file (default profiles/score_rate_<date>.jsonl)")
    args = ap.parse_args()
    L = scamd.lib()
    if L.sc_device_count() <= 0:
        raise SystemExit("no HIP device")
    hip = scamd.hip_runtime()
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    stream, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    bufs = []

    def alloc(nbytes):
        q = C.c_void_p()
        assert hip.hipMalloc(C.byref(q), max(int(nbytes), 1)) == 0
        bufs.append(q)
        return q

    p = lambda a: a.ctypes.data_as(C.c_void_p)
    engines = {prec: scamd.Engine(args.blocks, args.channels, seed=1, precision=prec) for prec in ("bf16", "fp8")}
    games = trace_set(engines["bf16"])
    mv, off, cm, cn, coff = scamd.pack_steps(games)
    P = int(off[-1])
    d = dict(boards=alloc(P * 7168), meta=alloc(P * 28), dist=alloc(P * 4672 * 4), dist_legal=alloc(P * 896), legal_idx=alloc(P * 448),
             n_legal=alloc(P * 4), status=alloc(len(games) * 4), outcome=alloc(P * 4), logp=alloc(P * 4672 * 4))
    rc = L.sc_encode_steps_device(engines["bf16"].h, 0, len(games), p(mv), p(off), p(cm), p(cn), p(coff), 0, 0, stream, d["boards"], d["meta"],
                                  d["dist"], d["dist_legal"], d["legal_idx"], d["n_legal"], d["status"])
    assert rc == 0, L.sc_last_error().decode()
    oc = np.zeros(P, np.float32)
    assert hip.hipMemcpy(d["outcome"], p(oc), oc.nbytes, 1) == 0
    assert hip.hipStreamSynchronize(stream) == 0
    outs = [alloc(P * 4) for _ in range(4)]
    summ = alloc(9 * 8)
    boards_h, meta_h, dist_h = np.zeros((P, 8, 8, 112), np.int8), np.zeros((P, 7), np.int32), np.zeros((P, 4672), np.float32)
    for dst, src in ((boards_h, d["boards"]), (meta_h, d["meta"]), (dist_h, d["dist"])):
        assert hip.hipMemcpy(p(dst), src, dst.nbytes, 2) == 0

    def timed(call):
        call()
        assert hip.hipStreamSynchronize(stream) == 0
        call_ms, dev_ms = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            hip.hipEventRecord(e0, stream)
            call()
            hip.hipEventRecord(e1, stream)
            assert hip.hipStreamSynchronize(stream) == 0
            call_ms.append((time.perf_counter() - t0) * 1e3)
            ms = C.c_float(0)
            hip.hipEventElapsedTime(C.byref(ms), e0, e1)
            dev_ms.append(ms.value)
        return statistics.median(call_ms), Ms(dev_ms)

    class Ms(float):
        """median of the regions, with the extremes"""
        def __new__(cls, xs):
            o = float.__new__(cls, statistics.median(xs))
            o.lo, o.hi = min(xs), max(xs)
            return o

    def row(c, dm, **more):
        r = {"call_ms": round(c, 3), "device_ms": round(dm, 3), "device_ms_min": round(dm.lo, 3), "device_ms_max": round(dm.hi, 3),
             "positions_per_s": round(P / (dm * 1e-3), 1)}
        r.update(more)
        return r

    forms = [f for f in args.forms.split(",") if f]

    def ok(rc):
        assert rc == 0, L.sc_last_error().decode()

    rows = {}
    for prec, eng in engines.items():
        r = {}
        fwd_c, fwd_d = timed(lambda: ok(L.sc_forward_device(eng.h, P, d["boards"], d["meta"], stream, None, outs[3])))
        fwdl_c, fwdl_d = timed(lambda: ok(L.sc_forward_device(eng.h, P, d["boards"], d["meta"], stream, d["logp"], outs[3])))
        r["forward_value_only"] = row(fwd_c, fwd_d)
        r["forward_with_logp"] = row(fwdl_c, fwdl_d)
        for form in ("dense", "sparse"):
            if form not in forms:
                continue
            dense = d["dist"] if form == "dense" else None
            sp = (d["dist_legal"], d["legal_idx"], d["n_legal"]) if form == "sparse" else (None, None, None)
            c, dm = timed(lambda: ok(L.sc_score_positions(eng.h, P, d["boards"], d["meta"], dense, sp[0], sp[1], sp[2], d["outcome"], stream,
                                                          outs[0], outs[1], outs[2], outs[3], summ)))
            r["score_" + form] = row(c, dm, x_forward_value_only=round(dm / fwd_d, 3))
        rows[prec] = r
        if args.no_host_route:
            continue
        # the route without the device entry points: forward to the host with the log-probabilities, float64 numpy there
        base = []
        for _ in range(max(2, args.reps // 3)):
            t0 = time.perf_counter()
            lp, v = eng.forward(boards_h, meta_h)
            t1 = time.perf_counter()
            l64 = lp.astype(np.float64)
            ce = -(np.where(dist_h != 0, dist_h * l64, 0.0)).sum(1)
            ent = -(np.exp(l64) * l64).sum(1)
            se = (v.astype(np.float64) - oc) ** 2
            _ = ce.mean(), ent.mean(), se.mean()
            base.append(((time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3))
        b_all, b_fwd = statistics.median(x[0] for x in base), statistics.median(x[1] for x in base)
        r["host_route"] = {"call_ms": round(b_all, 1), "forward_batch_ms": round(b_fwd, 1), "positions_per_s": round(P / (b_all * 1e-3), 1)}
        for form in ("dense", "sparse"):
            if "score_" + form in r:
                r[f"score_{form}_speedup_over_host_route"] = round(b_all / r["score_" + form]["call_ms"], 1)
    if "compare" in forms:
        c, dm = timed(lambda: ok(L.sc_compare_engines(engines["bf16"].h, engines["fp8"].h, P, d["boards"], d["meta"], stream, outs[0], outs[1], summ)))
        both = rows["bf16"]["forward_with_logp"]["device_ms"] + rows["fp8"]["forward_with_logp"]["device_ms"]
        s = np.zeros(9, np.float64)
        assert hip.hipMemcpy(p(s), summ, s.nbytes, 2) == 0
        rows["compare_bf16_fp8"] = row(c, dm, x_both_forward_with_logp=round(dm / both, 3), tv_mean=s[1], tv_max=s[3], dv_mean=s[5], dv_max=s[7])
    for q in bufs:
        hip.hipFree(q)
    for e in engines.values():
        e.close()
    line = json.dumps({"tool": "score_rate", "host": socket.gethostname(), "date": datetime.date.today().isoformat(), "games": len(games),
                       "plies": P, "net": f"{args.blocks}x{args.channels}", "reps": args.reps, "rows": rows})
    path = args.out or os.path.join(ROOT, "profiles", f"score_rate_{datetime.date.today().isoformat()}.jsonl")
    if path != os.devnull:
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "a") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
