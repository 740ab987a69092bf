"""Rate of the device-resident training-tensor path (sc_encode_steps_device) against the host path (sc_encode_steps), on the
256-game trace set of bench.py's encode_steps_rate.  Prints one JSON line.

  python tools/encode_device_rate.py [--reps 5]

device rows: the inputs are packed once (pack_steps) and the output buffers allocated once, outside the timing.
  call_ms     host wall time of the call plus the wait for its stream (upload of the traces, kernels)
  enqueue_ms  host wall time until the call returned (it does not synchronise)
  device_ms   HIP events recorded on the stream around the call (the same span as the GPU sees it)
host row: encode_steps_batch (Python packing + sc_encode_steps with its copy-out to pageable host memory) and the kernel time
sc_encode_steps_last_timing reports.  All figures are medians over --reps calls after one warm-up call."""
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

import numpy as np  # noqa: E402

import scamd  # noqa: E402


def trace_set(eng):
    """bench.py encode_steps_rate's games: 256 quick self-play games of the benchmark network"""
    quick = scamd.SelfPlay(eng, n_slots=256, n_games=256, rollout_num=8, num_steps=100, cpuct=2.5, temperature=0.0, temperature_switch=8,
                           epsilon=0.15, with_noise=True, seed=5, outcome_gate=10 ** 6)
    quick.run()
    games = []
    for g in range(256):
        tr = quick.trace(g)
        games.append([(s[0], [(c[0], c[1]) for c in s[2]]) for s in tr["steps"]])
    quick.close()
    return games


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--channels", type=int, default=128)
    args = ap.parse_args()
    L = scamd.lib()
    if L.sc_device_count() <= 0:
        raise SystemExit("no HIP device")
    eng = scamd.Engine(args.blocks, args.channels, seed=1)
    games = trace_set(eng)
    hip = scamd.hip_runtime()
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    stream, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0

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
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    bufs = []

    def alloc(nbytes):
        q = C.c_void_p()
        assert hip.hipMalloc(C.byref(q), max(int(nbytes), 1)) == 0
        bufs.append(q)
        return q

    status = alloc(len(games) * 4)
    lidx, nl = alloc(P * 448), alloc(P * 4)
    rows = {}
    for layout, lname in ((0, "reference"), (1, "trainer")):
        boards, meta = alloc(P * 7168 * (4 if layout else 1)), alloc(P * 28)
        for dist in ("legal", "dense"):
            d_dense = alloc(P * 4672 * 4) if dist == "dense" else None
            d_legal = alloc(P * 224 * 4) if dist == "legal" else None

            def call():
                rc = L.sc_encode_steps_device(eng.h, 0, len(games), p(mv), p(off), p(cm), p(cn), p(coff), 0, layout, stream, boards, meta,
                                              d_dense, d_legal, lidx, nl, status)
                assert rc == 0, L.sc_last_error().decode()
            call()
            assert hip.hipStreamSynchronize(stream) == 0
            call_ms, enq_ms, dev_ms = [], [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                hip.hipEventRecord(e0, stream)
                call()
                t1 = time.perf_counter()
                hip.hipEventRecord(e1, stream)
                assert hip.hipStreamSynchronize(stream) == 0
                t2 = time.perf_counter()
                ms = C.c_float(0)
                hip.hipEventElapsedTime(C.byref(ms), e0, e1)
                call_ms.append((t2 - t0) * 1e3)
                enq_ms.append((t1 - t0) * 1e3)
                dev_ms.append(ms.value)
            st = np.zeros(len(games), np.int32)
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            rc = hip.hipMemcpy(p(st), status, st.nbytes, 2)
            assert rc == 0, f"hipMemcpy: {rc}"
            if layout == 0 and dist == "dense":   # the device result is the host path's, bit for bit
                b = np.zeros((P, 8, 8, 112), np.int8)
                d = np.zeros((P, 4672), np.float32)
                assert hip.hipMemcpy(p(b), boards, b.nbytes, 2) == 0 and hip.hipMemcpy(p(d), d_dense, d.nbytes, 2) == 0
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
            c, dm = statistics.median(call_ms), statistics.median(dev_ms)
            rows[f"{lname}_{dist}"] = {"call_ms": round(c, 3), "enqueue_ms": round(statistics.median(enq_ms), 3), "device_ms": round(dm, 3),
                                       "plies_per_s": round(P / (c * 1e-3), 1), "device_plies_per_s": round(P / (dm * 1e-3), 1),
                                       "bytes_written_per_ply": out_b // P, "device_write_GBps": round(out_b / (dm * 1e-3) / 1e9, 1)}
    for q in bufs:
        hip.hipFree(q)
    hc, hk = statistics.median(host_call), statistics.median(host_k)
    print(json.dumps({"tool": "encode_device_rate", "host": socket.gethostname(), "date": datetime.date.today().isoformat(),
                      "games": len(games), "plies": P, "reps": args.reps, "device": rows,
                      "host_path": {"call_ms": round(hc, 3), "kernels_ms": round(hk, 3), "python_wall_ms": round(statistics.median(host_wall), 3),
                                    "plies_per_s": round(P / (hc * 1e-3), 1), "python_plies_per_s": round(P / (statistics.median(host_wall) * 1e-3), 1)}}))
    eng.close()


if __name__ == "__main__":
    main()
