"""Rate of scoring networks on device tensors (sc_score_positions in both dist forms, sc_compare_engines) on the 256-game trace
set of tools/ratelib.py, next to (a) the forward pass alone on the same positions (sc_forward_device without the
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
import time

import numpy as np

from ratelib import Hip, common_args, emit, ptr as p, record, require_device, spread, trace_set  # sets the package path

import scamd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    common_args(ap, reps=7)
    ap.add_argument("--forms", default="dense,sparse,compare", help="which calls to run (comma list of dense, sparse, compare)")
    ap.add_argument("--no-host-route", action="store_true", help="skip the sc_forward_batch + numpy baseline")
    ap.add_argument("--out", default=None, help="result file (default profiles/score_rate_<date>.jsonl)")
    args = ap.parse_args()
    L = require_device()
    hip = Hip(L)
    alloc, stream = hip.alloc, hip.stream
    engines = {prec: scamd.Engine(args.blocks, args.channels, seed=1, precision=prec) for prec in ("bf16", "fp8")}
    games = trace_set(engines["bf16"])
    mv, off, cm, cn, coff = scamd.pack_steps(games)
    P = int(off[-1])
    d = dict(boards=alloc(P * 7168), meta=alloc(P * 28), dist=alloc(P * 4672 * 4), dist_legal=alloc(P * 896), legal_idx=alloc(P * 448),
             n_legal=alloc(P * 4), status=alloc(len(games) * 4), outcome=hip.upload(np.zeros(P, np.float32)), logp=alloc(P * 4672 * 4))
    rc = L.sc_encode_steps_device(engines["bf16"].h, 0, len(games), p(mv), p(off), p(cm), p(cn), p(coff), 0, 0, stream, d["boards"], d["meta"],
                                  d["dist"], d["dist_legal"], d["legal_idx"], d["n_legal"], d["status"])
    assert rc == 0, L.sc_last_error().decode()
    hip.sync()
    oc = np.zeros(P, np.float32)
    outs = [alloc(P * 4) for _ in range(4)]
    summ = alloc(9 * 8)
    boards_h, meta_h = hip.download(d["boards"], (P, 8, 8, 112), np.int8), hip.download(d["meta"], (P, 7), np.int32)
    dist_h = hip.download(d["dist"], (P, 4672), np.float32)

    def measure(call):
        call_ms, _, dev_ms = hip.timed(call, args.reps)
        return spread(call_ms)[0], spread(dev_ms)

    def row(c, dm, **more):
        r = {"call_ms": round(c, 3), "device_ms": round(dm[0], 3), "device_ms_min": round(dm[1], 3), "device_ms_max": round(dm[2], 3),
             "positions_per_s": round(P / (dm[0] * 1e-3), 1)}
        r.update(more)
        return r

    forms = [f for f in args.forms.split(",") if f]
    rows = {}
    for prec, eng in engines.items():
        r = {}
        fwd_c, fwd_d = measure(lambda: L.sc_forward_device(eng.h, P, d["boards"], d["meta"], stream, None, outs[3]))
        fwdl_c, fwdl_d = measure(lambda: L.sc_forward_device(eng.h, P, d["boards"], d["meta"], stream, d["logp"], outs[3]))
        r["forward_value_only"] = row(fwd_c, fwd_d)
        r["forward_with_logp"] = row(fwdl_c, fwdl_d)
        for form in ("dense", "sparse"):
            if form not in forms:
                continue
            dense = d["dist"] if form == "dense" else None
            sp = (d["dist_legal"], d["legal_idx"], d["n_legal"]) if form == "sparse" else (None, None, None)
            c, dm = measure(lambda: L.sc_score_positions(eng.h, P, d["boards"], d["meta"], dense, sp[0], sp[1], sp[2], d["outcome"], stream,
                                                       outs[0], outs[1], outs[2], outs[3], summ))
            r["score_" + form] = row(c, dm, x_forward_value_only=round(dm[0] / fwd_d[0], 3))
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
        b_all, b_fwd = spread([x[0] for x in base])[0], spread([x[1] for x in base])[0]
        r["host_route"] = {"call_ms": round(b_all, 1), "forward_batch_ms": round(b_fwd, 1), "positions_per_s": round(P / (b_all * 1e-3), 1)}
        for form in ("dense", "sparse"):
            if "score_" + form in r:
                r[f"score_{form}_speedup_over_host_route"] = round(b_all / r["score_" + form]["call_ms"], 1)
    if "compare" in forms:
        c, dm = measure(lambda: L.sc_compare_engines(engines["bf16"].h, engines["fp8"].h, P, d["boards"], d["meta"], stream, outs[0], outs[1], summ))
        both = rows["bf16"]["forward_with_logp"]["device_ms"] + rows["fp8"]["forward_with_logp"]["device_ms"]
        s = hip.download(summ, 9, np.float64)
        rows["compare_bf16_fp8"] = row(c, dm, x_both_forward_with_logp=round(dm[0] / both, 3), tv_mean=s[1], tv_max=s[3], dv_mean=s[5], dv_max=s[7])
    hip.close()
    for e in engines.values():
        e.close()
    emit([record("score_rate", games=len(games), plies=P, net=f"{args.blocks}x{args.channels}", reps=args.reps, rows=rows)], args.out, "score_rate")


if __name__ == "__main__":
    main()
