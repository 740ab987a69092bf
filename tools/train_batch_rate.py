"""Rate of building trainer-layout minibatches from the compact tensors: sc_gather_batch (k_gather_batch, one launch) next to the
route that exists without it -- four torch ops on the same tensors (index_select, permute + float, zeros, scatter_add_) -- in the
same visit, on the 256-game trace set of tools/ratelib.py.  Appends one JSON line per row to
profiles/train_batch_rate_<date>.jsonl and prints them.

  python tools/train_batch_rate.py [--reps 7] [--iters 20] [--batches 1024,8192]

Every figure is the median over --reps regions after a warm-up region, with the smallest and largest region next to it (ms_min /
ms_max): HIP events (torch.cuda.Event) on the caller's stream around --iters calls, divided by --iters.  Rows per batch size B:

  gather_call    sc_gather_batch into buffers allocated once (the kernel and its launch)
  gather_torch   scamd.gather_batch_torch (the same plus four torch.empty)
  torch_route    the torch composition (it allocates its results too)

Per sample 8 548 B are read and 47 392 B written; hbm_frac is that traffic over the time against the 8 TB/s bench.py uses, and
hbm_bound_ms the time it would take at that rate.  launch_floor_ms is gather_call at B = 1: one workgroup's chain of dependent
loads and stores plus the launch -- the bound that applies where B workgroups do not fill the GPU for long.  The two routes'
results are compared bit for bit before anything is timed."""
import argparse
import ctypes as C

import torch  # before scamd: one HIP runtime in the process

from ratelib import common_args, emit, record, require_device, spread, timed_torch, trace_set  # sets the package path

import scamd  # noqa: E402

HBM_PEAK_GBS = 8000.0   # bench.py's figure
READ_B, WRITE_B = 8548, 47392


def torch_route(src, rows):
    """the composition include/sc_engine.h describes: three passes over the batch"""
    r = rows.long()
    boards = src["boards"].index_select(0, r).permute(0, 3, 1, 2).to(torch.float32, memory_format=torch.contiguous_format)
    meta = src["meta"].index_select(0, r).float()
    dist = torch.zeros((r.shape[0], 4672), dtype=torch.float32, device=r.device)
    dist.scatter_add_(1, src["legal_idx"].index_select(0, r).long(), src["dist_legal"].index_select(0, r))
    return boards, meta, dist, src["outcome"].index_select(0, r)[:, None]


def main():
    ap = argparse.ArgumentParser()
    common_args(ap, reps=7)
    ap.add_argument("--iters", type=int, default=20, help="calls per timed region")
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--out", default=None, help="result file (default profiles/train_batch_rate_<date>.jsonl)")
    args = ap.parse_args()
    L = require_device()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    eng = scamd.Engine(args.blocks, args.channels, seed=1)
    games = trace_set(eng)
    src = scamd.encode_steps_torch(scamd.pack_steps(games), layout="reference", dist="legal", engine=eng)
    assert (src["status"] == 0).all()
    P = int(src["boards"].shape[0])
    stream = torch.cuda.current_stream(0)
    tp = lambda t: C.c_void_p(t.data_ptr())

    def measure(call):
        return spread(timed_torch(call, args.reps, args.iters, stream))

    def raw_call(rows, outs):
        B = int(rows.shape[0])

        def call():
            rc = L.sc_gather_batch(0, P, B, tp(rows), None, tp(src["boards"]), tp(src["meta"]), tp(src["dist_legal"]), tp(src["legal_idx"]),
                                   tp(src["n_legal"]), tp(src["outcome"]), C.c_void_p(stream.cuda_stream), tp(outs[0]), tp(outs[1]),
                                   tp(outs[2]), tp(outs[3]), None)
            assert rc == 0, L.sc_last_error().decode()
        return call

    def outputs(B):
        return [torch.empty(s, dtype=torch.float32, device=dev) for s in ((B, 112, 8, 8), (B, 7), (B, 4672), (B, 1))]

    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    one = torch.zeros(1, dtype=torch.int32, device=dev)
    floor = measure(raw_call(one, outputs(1)))
    lines = []
    base = record("train_batch_rate", games=len(games), plies=P, reps=args.reps, calls_per_region=args.iters, read_bytes_per_sample=READ_B,
                  write_bytes_per_sample=WRITE_B, launch_floor_ms=round(floor[0], 5))
    for B in (int(x) for x in args.batches.split(",") if x):
        rows = (torch.randperm(P, generator=gen, device=dev)[:B] if B <= P else torch.randint(0, P, (B,), generator=gen, device=dev)).to(torch.int32)
        got, ref = scamd.gather_batch_torch(src, rows), torch_route(src, rows)
        equal = all(torch.equal(a, b) for a, b in zip(got, ref))
        outs = outputs(B)
        res = {"gather_call": measure(raw_call(rows, outs)), "gather_torch": measure(lambda: scamd.gather_batch_torch(src, rows)),
               "torch_route": measure(lambda: torch_route(src, rows))}
        hbm_bound = B * (READ_B + WRITE_B) / (HBM_PEAK_GBS * 1e9) * 1e3
        t_med, t_lo, t_hi = res["torch_route"]
        for name, (med, lo, hi) in res.items():
            line = dict(base, row=name, batch=B, ms=round(med, 5), ms_min=round(lo, 5), ms_max=round(hi, 5),
                        samples_per_s=round(B / (med * 1e-3), 1), hbm_frac=round(hbm_bound / med, 4), hbm_bound_ms=round(hbm_bound, 5),
                        bound="launch" if floor[0] > hbm_bound else "hbm", equal_to_torch_route=equal)
            if name != "torch_route":
                # done when the median is no longer than the torch route's; the margin is that route's own spread
                line.update(x_torch_route=round(med / t_med, 4), torch_route_spread_ms=round(t_hi - t_lo, 5),
                            no_slower_than_torch_route=bool(med <= t_med + (t_hi - t_lo)))
            lines.append(line)
    eng.close()
    emit(lines, args.out, "train_batch_rate")


if __name__ == "__main__":
    main()
