"""Rate of merging identical training positions: sc_merge_positions (csrc/merge_kernels.hip) next to the route that exists without
it -- torch.unique(dim=0, return_inverse=True) over the rows' sample bytes, then index_add_ and a division -- in the same visit,
on the plies of the 256-game trace set of tools/ratelib.py.  Appends one JSON line per row to
profiles/merge_rate_<date>.jsonl and prints them.

  python tools/merge_rate.py [--reps 7] [--iters 5]

Every figure is the median over --reps regions after a warm-up region, with the smallest and largest region next to it (ms_min /
ms_max): HIP events (torch.cuda.Event) on the caller's stream around --iters calls, divided by --iters.  Rows:

  merge_call     sc_merge_positions into buffers and a workspace allocated once (every kernel of the call, no host read)
  merge_torch    scamd.replay.merge_positions_torch (the same plus its allocations and the host read of the counts)
  torch_route    the torch composition (it allocates its results too; its sums are atomic, their order is not fixed)

hbm_bound_ms is the time 8 548 B per position take at the 8 TB/s bench.py uses (the rows are read once by the key kernel; the
compare and the merge read again what is then in the caches).  The two routes' partitions are compared before anything is timed.
The last line is the diversity report of the run (scamd.replay.unique_by_ply): plies and distinct samples per ply index."""
import argparse
import ctypes as C

import torch  # before scamd: one HIP runtime in the process

from ratelib import common_args, emit, record, require_device, spread, timed_torch, trace_set  # sets the package path

import scamd  # noqa: E402
from scamd import replay  # noqa: E402

HBM_PEAK_GBS = 8000.0   # bench.py's figure
PLY_B = 8548
KEYS = ("boards", "meta", "dist_legal", "legal_idx", "n_legal", "outcome")


def torch_route(src):
    """-> (group of each position in torch.unique's order, mean shares [G][224], mean outcome [G])"""
    n = src["boards"].shape[0]
    nl = src["n_legal"]
    li = src["legal_idx"].clone()
    li[torch.arange(224, device=li.device)[None, :] >= nl[:, None]] = 0   # the padding is not part of the sample
    as_bytes = lambda t: t.reshape(n, -1).view(torch.uint8)
    sample = torch.cat([as_bytes(src["boards"]), as_bytes(src["meta"]), as_bytes(nl), as_bytes(li)], dim=1)
    uniq, inv = torch.unique(sample, dim=0, return_inverse=True)
    G = uniq.shape[0]
    cnt = torch.zeros(G, dtype=torch.float32, device=inv.device).index_add_(0, inv, torch.ones(n, dtype=torch.float32, device=inv.device))
    dist = torch.zeros((G, 224), dtype=torch.float32, device=inv.device).index_add_(0, inv, src["dist_legal"])
    oc = torch.zeros(G, dtype=torch.float32, device=inv.device).index_add_(0, inv, src["outcome"])
    return inv, dist / cnt[:, None], oc / cnt


def by_first_position(inv):
    """a partition's labels renumbered by ascending smallest position: sc_merge_positions' numbering"""
    n, G = inv.shape[0], int(inv.max()) + 1
    first = torch.full((G,), n, dtype=torch.int64, device=inv.device).scatter_reduce_(0, inv, torch.arange(n, device=inv.device), "amin")
    rank = torch.empty(G, dtype=torch.int64, device=inv.device)
    rank[torch.argsort(first)] = torch.arange(G, device=inv.device)
    return rank[inv]


def main():
    ap = argparse.ArgumentParser()
    common_args(ap, reps=7)
    ap.add_argument("--iters", type=int, default=5, help="calls per timed region")
    ap.add_argument("--out", default=None, help="result file (default profiles/merge_rate_<date>.jsonl)")
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

    # the two partitions are equal, and the means agree to float32 rounding (the torch route's sums have no fixed order)
    m = replay.merge_positions_torch(src)
    inv, t_dist, t_oc = torch_route(src)
    G = int(m["count"].shape[0])
    assert m["n_bad"] == 0 and m["n_key_clash"] == 0
    equal = bool(torch.equal(by_first_position(inv), m["group_of"].long()))
    assert equal, "the partitions differ"
    head = inv[m["first"].long()]
    live = torch.arange(224, device=dev)[None, :] < m["n_legal"][:, None]
    max_diff = float(((m["dist_legal"] - t_dist[head]).abs() * live).max())
    tol = int(m["count"].max()) * 2.0 ** -23   # shares and outcomes within [-1, 1]: m additions in another order, half an ulp of 1 each way
    assert max_diff <= tol and float((m["outcome"] - t_oc[head]).abs().max()) <= tol

    def measure(call):
        return spread(timed_torch(call, args.reps, args.iters, stream))

    need = C.c_size_t(0)
    assert L.sc_merge_positions_workspace(P, C.byref(need)) == 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    outs = [torch.empty_like(src[k]) for k in KEYS] + [torch.empty(P, dtype=torch.int32, device=dev) for _ in range(3)]
    counts = torch.empty(4, dtype=torch.int32, device=dev)

    def raw_call():
        rc = L.sc_merge_positions(0, P, P, None, *[tp(src[k]) for k in KEYS], 128, tp(ws), need.value, C.c_void_p(stream.cuda_stream),
                                  *[tp(o) for o in outs], tp(counts))
        assert rc == 0, L.sc_last_error().decode()

    res = {"merge_call": measure(raw_call), "merge_torch": measure(lambda: replay.merge_positions_torch(src)),
           "torch_route": measure(lambda: torch_route(src))}
    hbm_bound = P * PLY_B / (HBM_PEAK_GBS * 1e9) * 1e3
    base = record("merge_rate", games=len(games), plies=P, groups=G, duplicate_share=round(1 - G / P, 5), largest_group=int(m["count"].max()),
                  reps=args.reps, calls_per_region=args.iters, bytes_per_ply=PLY_B, workspace_bytes=need.value,
                  hbm_bound_ms=round(hbm_bound, 5), partitions_equal=equal, max_abs_diff_to_torch_means=max_diff)
    t_med, t_lo, t_hi = res["torch_route"]
    lines = []
    for name, (med, lo, hi) in res.items():
        line = dict(base, row=name, ms=round(med, 5), ms_min=round(lo, 5), ms_max=round(hi, 5), plies_per_s=round(P / (med * 1e-3), 1),
                    x_hbm_bound=round(med / hbm_bound, 2))
        if name != "torch_route":
            line.update(x_torch_route=round(med / t_med, 4), torch_route_spread_ms=round(t_hi - t_lo, 5))
        lines.append(line)
    u = replay.unique_by_ply(m)
    lines.append(dict(tool="merge_rate", row="unique_by_ply", date=base["date"], games=len(games), plies=u["plies"].tolist(),
                      distinct=u["distinct"].tolist()))
    eng.close()
    emit(lines, args.out, "merge_rate")


if __name__ == "__main__":
    main()
