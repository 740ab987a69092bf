"""What the rate tools share (tools/*_rate.py, tools/match_time.py): the package path and the device check, the common arguments,
the 256-game trace set, device buffers with the event-timed loop on the engine's HIP runtime (Hip: no torch), the same loop on
torch events (timed_torch), and the result record and its writer.  A new rate tool starts from these: one timing loop, so that
a figure can be compared with the files in profiles/.  No torch at module level: a tool that needs torch imports it first."""
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


def require_device():
    """scamd.lib(), or the exit every tool makes without a device"""
    L = scamd.lib()
    if L.sc_device_count() <= 0:
        raise SystemExit("no HIP device")
    return L


def common_args(ap, reps, blocks=10, channels=128):
    ap.add_argument("--reps", type=int, default=reps)
    ap.add_argument("--blocks", type=int, default=blocks)
    ap.add_argument("--channels", type=int, default=channels)


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


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Hip:
    """device buffers, one non-default stream and two events on the engine's HIP runtime"""

    def __init__(self, L, hip=None):
        self.L, self.hip = L, hip or scamd.hip_runtime()
        self.stream, self.e0, self.e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert self.hip.hipStreamCreate(C.byref(self.stream)) == 0
        assert self.hip.hipEventCreate(C.byref(self.e0)) == 0 and self.hip.hipEventCreate(C.byref(self.e1)) == 0
        self.bufs = []

    def alloc(self, nbytes):
        q = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(q), max(int(nbytes), 1)) == 0
        self.bufs.append(q)
        return q

    def upload(self, a):
        a = np.ascontiguousarray(a)
        q = self.alloc(a.nbytes)
        assert self.hip.hipMemcpy(q, ptr(a), a.nbytes, 1) == 0
        return q

    def download(self, q, shape, dtype):
        a = np.zeros(shape, dtype)
        assert self.hip.hipMemcpy(ptr(a), q, a.nbytes, 2) == 0
        return a

    def sync(self):
        assert self.hip.hipStreamSynchronize(self.stream) == 0

    def close(self):
        for q in self.bufs:
            self.hip.hipFree(q)
        self.bufs = []
        self.hip.hipEventDestroy(self.e0)
        self.hip.hipEventDestroy(self.e1)
        self.hip.hipStreamDestroy(self.stream)

    def timed(self, call, reps):
        """one checked warm-up call, then `reps` regions of one call -> (call_ms, enqueue_ms, device_ms), `reps` samples each:
        host wall time of the call plus the wait for the stream, host wall time until the call returned, and HIP events recorded on
        the stream around the call.  `call` returns the entry point's code"""
        hip, stream, e0, e1 = self.hip, self.stream, self.e0, self.e1
        rc = call()
        assert rc == 0, self.L.sc_last_error().decode()
        self.sync()
        call_ms, enq_ms, dev_ms = [], [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            hip.hipEventRecord(e0, stream)
            rc = call()
            assert rc == 0, self.L.sc_last_error().decode()
            t1 = time.perf_counter()
            hip.hipEventRecord(e1, stream)
            assert hip.hipStreamSynchronize(stream) == 0
            t2 = time.perf_counter()
            ms = C.c_float(0)
            hip.hipEventElapsedTime(C.byref(ms), e0, e1)
            call_ms.append((t2 - t0) * 1e3)
            enq_ms.append((t1 - t0) * 1e3)
            dev_ms.append(ms.value)
        return call_ms, enq_ms, dev_ms


def timed_torch(call, reps, iters, stream):
    """a warm-up region of `iters` calls, then `reps` regions of `iters` calls between torch events on `stream` -> ms per call"""
    import torch
    for _ in range(iters):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(iters):
            call()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return ms


def spread(xs):
    """(median, min, max)"""
    return statistics.median(xs), min(xs), max(xs)


def record(tool, **fields):
    return dict(tool=tool, host=socket.gethostname(), date=datetime.date.today().isoformat(), **fields)


def emit(lines, out, tool, mode="a"):
    """prints the records and appends them to `out` (None: profiles/<tool>_<date>.jsonl); os.devnull: prints only"""
    text = "\n".join(json.dumps(ln) for ln in lines)
    print(text, flush=True)
    path = out or os.path.join(ROOT, "profiles", f"{tool}_{datetime.date.today().isoformat()}.jsonl")
    if path != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, mode) as f:
            f.write(text + "\n")
