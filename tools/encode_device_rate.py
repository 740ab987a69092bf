"""Rate of the device-resident training-tensor path (sc_encode_steps_device) against the host path (sc_encode_steps), on the
256-game trace set of bench.py's encode_steps_rate.  Prints one JSON line and appends it to
profiles/encode_device_rate_<date>.jsonl (--out).

  python tools/encode_device_rate.py [--reps 5] [--out FILE]

device rows: the inputs are packed once (pack_steps) and the output buffers allocated once, outside the timing.
  call_ms     host wall time of the call plus the wait for its stream (upload of the traces, kernels)
  enqueue_ms  host wall time until the call returned (it does not synchronise)
  device_ms   HIP events recorded on the stream around the call (the same span as the GPU sees it)
host row: encode_steps_batch (Python packing + sc_encode_steps with its copy-out to pageable host memory) and the kernel time
sc_encode_steps_last_timing reports.  All figures are medians over --reps calls after one warm-up call."""
import argparse
import time

import numpy as np

from ratelib import Hip, common_args, emit, ptr as p, record, require_device, spread, trace_set  # sets the package path

import scamd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    common_args(ap, reps=5)
    ap.add_argument("--out", default=None, help="result file (default profiles/encode_device_rate_<date>.jsonl)")
    args = ap.parse_args()
    L = require_device()
    eng = scamd.Engine(args.blocks, args.channels, seed=1)
    games = trace_set(eng)
    hip = Hip(L)
    alloc, stream = hip.alloc, hip.stream

    # host path
    scamd.encode_steps_batch(games[:8], engine=eng)
    host_wall, host_call, host_k = [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        r = scamd.encode_steps_batch(games, engine=eng)
        host_wall.append((time.perf_counter() - t0) * 1e3)
        k, c = scamd.binding.encode_steps_last_timing()
        host_k.append(k)
        host_call.append(c)
    P = int(r["ply_off"][-1])
    assert (r["status"] == 0).all()

    mv, off, cm, cn, coff = scamd.pack_steps(games)
    status = alloc(len(games) * 4)
    lidx, nl = alloc(P * 448), alloc(P * 4)
    rows = {}
    for layout, lname in ((0, "reference"), (1, "trainer")):
        boards, meta = alloc(P * 7168 * (4 if layout else 1)), alloc(P * 28)
        for dist in ("legal", "dense"):
            d_dense = alloc(P * 4672 * 4) if dist == "dense" else None
            d_legal = alloc(P * 224 * 4) if dist == "legal" else None
            call_ms, enq_ms, dev_ms = hip.timed(lambda: L.sc_encode_steps_device(
                eng.h, 0, len(games), p(mv), p(off), p(cm), p(cn), p(coff), 0, layout, stream, boards, meta, d_dense, d_legal, lidx, nl,
                status), args.reps)
            st = hip.download(status, len(games), np.int32)
            if layout == 0 and dist == "dense":   # the device result is the host path's, bit for bit
                b, d = hip.download(boards, (P, 8, 8, 112), np.int8), hip.download(d_dense, (P, 4672), np.float32)
                bad_b = np.nonzero((b != r["boards"]).reshape(P, -1).any(1))[0]
                bad_d = np.nonzero((d.view(np.uint32) != r["dist"].view(np.uint32)).any(1))[0]
                if bad_b.size or bad_d.size:
                    raise SystemExit(f"device result differs from the host path: boards of {bad_b.size} plies {bad_b[:8].tolist()}, "
                                     f"dist of {bad_d.size} plies {bad_d[:8].tolist()}")
            if not np.array_equal(st, r["status"]):
                bad = np.nonzero(st != r["status"])[0]
                raise SystemExit(f"{lname}/{dist}: status differs from the host path in {bad.size} games, e.g. "
                                 f"{[(int(g), int(st[g]), int(r['status'][g])) for g in bad[:8]]}")
            out_b = P * (7168 * (4 if layout else 1) + 28 + (4672 * 4 if dist == "dense" else 224 * 4) + 448 + 4)
            c, dm = spread(call_ms)[0], spread(dev_ms)[0]
            rows[f"{lname}_{dist}"] = {"call_ms": round(c, 3), "enqueue_ms": round(spread(enq_ms)[0], 3), "device_ms": round(dm, 3),
                                       "plies_per_s": round(P / (c * 1e-3), 1), "device_plies_per_s": round(P / (dm * 1e-3), 1),
                                       "bytes_written_per_ply": out_b // P, "device_write_GBps": round(out_b / (dm * 1e-3) / 1e9, 1)}
    hip.close()
    hc, hk, hw = spread(host_call)[0], spread(host_k)[0], spread(host_wall)[0]
    emit([record("encode_device_rate", games=len(games), plies=P, reps=args.reps, device=rows,
                 host_path={"call_ms": round(hc, 3), "kernels_ms": round(hk, 3), "python_wall_ms": round(hw, 3),
                            "plies_per_s": round(P / (hc * 1e-3), 1), "python_plies_per_s": round(P / (hw * 1e-3), 1)})],
         args.out, "encode_device_rate")
    eng.close()


if __name__ == "__main__":
    main()
