"""Recorded games -> training tensors, and networks judged on them, on the GPU (csrc/encode_steps.hip, csrc/device_calls.hip)."""
import numpy as np

from .binding import MAX_MOVES, EngineError, _check, _moves, _p, _stream, _torch, _tp, lib
from .net import _check_reference_tensors

_LAYOUTS = {"reference": 0, "trainer": 1}
_DISTS = ("dense", "legal", "both")
SCORE_SUMMARY = ("n", "loss1", "loss2", "pi_entropy", "n_nonfinite")
COMPARE_SUMMARY = ("n", "tv_mean", "tv_std", "tv_max", "tv_min", "dv_mean", "dv_std", "dv_max", "dv_min")


def pack_steps(games):
    """The list form of encode_steps_batch -> the packed arrays (moves, move_off, child_mv, child_n, child_off) that
    sc_encode_steps / sc_encode_steps_device take"""
    n = len(games)
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum([len(g) for g in games])
    P = int(off[n])
    flat = _moves([s[0] for g in games for s in g])
    coff = np.zeros(P + 1, np.uint32)
    coff[1:] = np.cumsum([len(s[1]) for g in games for s in g])
    cm = _moves([c[0] for g in games for s in g for c in s[1]])
    cn = np.asarray([int(c[1]) for g in games for s in g for c in s[1]] or [0], np.uint32)
    return flat, off, cm, cn, coff


def encode_steps_batch(games, apply_mirror=False, device=0, engine=None):
    """Trace -> training tensors for a batch of games on the GPU (sc_encode_steps).
    games: list of step lists [(next_move, [(move, count), ...]), ...] with moves as uint16 or UCI strings -- the
    `steps` argument of libsmartchess.chess_encode_steps (reference src/lib.rs:46-50), one per game.
    -> dict(boards int8[P,8,8,112], meta int32[P,7], dist f32[P,4672], move_indices [P lists], ply_off[n+1], status[n])"""
    L = lib()
    flat, off, cm, cn, coff = pack_steps(games)
    n, P = len(games), int(off[-1])
    boards = np.zeros((max(P, 1), 8, 8, 112), np.int8)
    meta = np.zeros((max(P, 1), 7), np.int32)
    dist = np.zeros((max(P, 1), 4672), np.float32)
    li = np.zeros((max(P, 1), MAX_MOVES), np.uint16)
    nl = np.zeros(max(P, 1), np.int32)
    status = np.zeros(max(n, 1), np.int32)
    _check(L.sc_encode_steps(engine.h if engine else None, device, n, _p(flat), _p(off), _p(cm), _p(cn), _p(coff),
                             int(bool(apply_mirror)), _p(boards), _p(meta), _p(dist), _p(li), _p(nl), _p(status)))
    return dict(boards=boards[:P], meta=meta[:P], dist=dist[:P], move_indices=[li[i, :nl[i]].astype(np.int32) for i in range(P)],
                ply_off=off, status=status[:n])


def encode_steps(steps, apply_mirror=False, device=0, engine=None):
    """Mirror of libsmartchess.chess_encode_steps(steps, apply_mirror) (reference src/lib.rs:46-128, used by
    py/dataset.py:77): one game -> [(boards int8[8,8,112], meta int32[7], dist f32[4672], move_indices), ...].
    Raises EngineError where the reference panics (children != legal moves, or an illegal played move)."""
    r = encode_steps_batch([steps], apply_mirror, device, engine)
    st = int(r["status"][0])
    if st >= 1000:
        raise EngineError(f"inconsistent moves at ply {st - 1000}")
    if st < 0:
        raise EngineError(f"num_act table doesn't include the next move (ply {-st - 1})")
    return [(r["boards"][i], r["meta"][i], r["dist"][i], r["move_indices"][i]) for i in range(len(steps))]


def _device_outputs(torch, device, P, n, layout, dist):
    if layout not in _LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(_LAYOUTS)}")
    if dist not in _DISTS:
        raise ValueError(f"dist must be one of {_DISTS}")
    lay = _LAYOUTS[layout]
    dev = torch.device("cuda", device)
    R = max(P, 1)
    out = {}
    if lay == 1:
        out["boards"] = torch.empty((R, 112, 8, 8), dtype=torch.float32, device=dev)
        out["meta"] = torch.empty((R, 7), dtype=torch.float32, device=dev)
    else:
        out["boards"] = torch.empty((R, 8, 8, 112), dtype=torch.int8, device=dev)
        out["meta"] = torch.empty((R, 7), dtype=torch.int32, device=dev)
    out["dist"] = torch.empty((R, 4672), dtype=torch.float32, device=dev) if dist in ("dense", "both") else None
    out["dist_legal"] = torch.empty((R, MAX_MOVES), dtype=torch.float32, device=dev) if dist in ("legal", "both") else None
    out["legal_idx"] = torch.empty((R, MAX_MOVES), dtype=torch.int16, device=dev)   # action indices < 4672: exact in int16
    out["n_legal"] = torch.empty(R, dtype=torch.int32, device=dev)
    out["status"] = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    args = [lay] + [_tp(out[k]) for k in ("boards", "meta", "dist", "dist_legal", "legal_idx", "n_legal", "status")]
    return out, args


def _finish_outputs(torch, out, ply_off, outcome_per_game, apply_mirror, device):
    n = ply_off.size - 1
    P = int(ply_off[n])
    status = out.pop("status")[:n].cpu().numpy()   # the one host copy: waits for the work on the current stream
    res = {k: (None if v is None else v[:P]) for k, v in out.items()}
    oc = np.repeat(np.asarray(outcome_per_game, np.float32), np.diff(ply_off.astype(np.int64)))
    if apply_mirror:
        oc = -oc   # ChessDataset negates the outcome under the mirror (py/dataset.py)
    res["outcome"] = torch.from_numpy(oc).to(torch.device("cuda", device))
    res["ply_off"] = ply_off
    res["status"] = status
    return res


def encode_steps_torch(games, apply_mirror=False, layout="trainer", dist="dense", engine=None, device=0, outcomes=None):
    """Training tensors on the GPU, for a trainer there (sc_encode_steps_device): no copy through the host.
    games: the list form of encode_steps_batch, or the packed arrays (moves, move_off, child_mv, child_n, child_off) as a
    tuple or a dict with those keys (pack_steps).  layout "trainer": boards float32 [P,112,8,8] and meta float32 [P,7]
    (py/dataset.py _prepare); "reference": int8 [P,8,8,112] and int32 [P,7] as encode_steps_batch.  dist "dense": dist
    float32 [P,4672]; "legal": dist_legal float32 [P,224] aligned with legal_idx (rebuild the dense rows with
    zeros(P, 4672).scatter_add_(1, legal_idx.long(), dist_legal) -- scatter_add_, not scatter_: padding entries point at action
    0); "both".  outcomes: per game, White's result (1, -1, 0; None: 0) -> outcome float32 [P], negated under apply_mirror as
    ChessDataset does.
    -> dict of torch tensors on cuda:<device> (enqueued on torch.cuda.current_stream()): boards, meta, dist, dist_legal,
    legal_idx (int16) [P,224], n_legal int32 [P], outcome; plus ply_off (numpy) and status (numpy, sc_encode_steps's codes)."""
    torch = _torch()   # first: without a GPU this raises before the arguments are looked at
    L = lib()
    if isinstance(games, dict):
        packed = tuple(games[k] for k in ("moves", "move_off", "child_mv", "child_n", "child_off"))
    elif isinstance(games, tuple) and len(games) == 5 and all(isinstance(a, np.ndarray) for a in games):
        packed = games
    else:
        packed = pack_steps(games)
    flat, off, cm, cn, coff = (np.ascontiguousarray(a, t) for a, t in zip(packed, (np.uint16, np.uint32, np.uint16, np.uint32, np.uint32)))
    n = off.size - 1
    dev = engine.device if engine is not None else device
    out, args = _device_outputs(torch, dev, int(off[n]), n, layout, dist)
    _check(L.sc_encode_steps_device(engine.h if engine else None, dev, n, _p(flat if flat.size else np.zeros(1, np.uint16)), _p(off),
                                    _p(cm if cm.size else np.zeros(1, np.uint16)), _p(cn if cn.size else np.zeros(1, np.uint32)),
                                    _p(coff), int(bool(apply_mirror)), args[0], _stream(torch, dev), *args[1:]))
    oc = np.zeros(n, np.float32) if outcomes is None else np.asarray(outcomes, np.float32)
    return _finish_outputs(torch, out, off, oc, apply_mirror, dev)


def _sparse_dtypes_ok(torch, dist_legal, legal_idx, n_legal):
    """the sparse visit shares as the encoder writes them: float32, int16 (or uint16), int32"""
    return (dist_legal.dtype, n_legal.dtype) == (torch.float32, torch.int32) and legal_idx.dtype in (torch.int16, getattr(torch, "uint16", torch.int16))


def score_torch(engine, tensors):
    """A network judged on recorded search results (sc_score_positions; the reference's validation_step and pi_entropy).
    tensors: the dict encode_steps_torch(..., layout="reference") / SelfPlay.training_tensors(..., layout="reference")
    returns -- boards, meta, outcome and the visit shares as dist (dense) or dist_legal + legal_idx + n_legal (with
    dist="both" the sparse form is used: 21 x fewer bytes).
    -> dict: per-position torch tensors ce, se, ent, value (float32 [P], on the GPU), floats loss1 = mean ce, loss2 = mean se,
    pi_entropy = mean ent, ints n and n_nonfinite (positions whose ce, se or ent is not finite; they stay in the means).
    Enqueued on torch.cuda.current_stream(); the summary's copy to the host waits for it."""
    torch = _torch()
    boards, meta = tensors["boards"], tensors["meta"]
    n = _check_reference_tensors(torch, boards, meta, engine.device)
    dist, dl, li, nl = (tensors.get(k) for k in ("dist", "dist_legal", "legal_idx", "n_legal"))
    if dl is not None and li is not None and nl is not None:
        dist = None
        if not _sparse_dtypes_ok(torch, dl, li, nl):
            raise ValueError("dist_legal float32, legal_idx int16 and n_legal int32 are needed")
        sparse = (dl, li, nl)
    elif dist is not None:
        if dist.dtype != torch.float32:
            raise ValueError("dist: float32 is needed")
        sparse = (None, None, None)
    else:
        raise ValueError("the visit shares are missing: dist, or dist_legal + legal_idx + n_legal")
    outcome = tensors["outcome"]
    dev = torch.device("cuda", engine.device)
    for name, t, rows in (("dist", dist, n), ("dist_legal", sparse[0], n), ("legal_idx", sparse[1], n), ("n_legal", sparse[2], n),
                          ("outcome", outcome, n)):
        if t is not None and (t.device != dev or not t.is_contiguous() or t.shape[0] != rows):
            raise ValueError(f"{name}: a contiguous tensor of {rows} rows on cuda:{engine.device} is needed")
    if outcome.dtype != torch.float32:
        raise ValueError("outcome: float32 is needed")
    out = {k: torch.empty(n, dtype=torch.float32, device=dev) for k in ("ce", "se", "ent", "value")}
    summary = torch.empty(len(SCORE_SUMMARY), dtype=torch.float64, device=dev)
    _check(engine.L.sc_score_positions(engine.h, n, _tp(boards), _tp(meta), _tp(dist), _tp(sparse[0]), _tp(sparse[1]), _tp(sparse[2]),
                                       _tp(outcome), _stream(torch, engine.device), _tp(out["ce"]), _tp(out["se"]), _tp(out["ent"]),
                                       _tp(out["value"]), _tp(summary)))
    s = summary.cpu().tolist()
    out.update(n=int(s[0]), loss1=s[1], loss2=s[2], pi_entropy=s[3], n_nonfinite=int(s[4]))
    return out


def compare_torch(engine_a, engine_b, tensors):
    """Agreement of two networks on the same positions (sc_compare_engines; the reference's scripts/validate_model.py).
    tensors: a dict with boards and meta in layout="reference" on the engines' GPU.
    -> dict: per-position torch tensors tv (total variation of the two policies) and dv (|value_a - value_b|), and the floats
    tv_mean, tv_std, tv_max, tv_min, dv_mean, dv_std, dv_max, dv_min (population standard deviation), int n."""
    torch = _torch()
    boards, meta = tensors["boards"], tensors["meta"]
    n = _check_reference_tensors(torch, boards, meta, engine_a.device)
    dev = torch.device("cuda", engine_a.device)
    out = {k: torch.empty(n, dtype=torch.float32, device=dev) for k in ("tv", "dv")}
    summary = torch.empty(len(COMPARE_SUMMARY), dtype=torch.float64, device=dev)
    _check(engine_a.L.sc_compare_engines(engine_a.h, engine_b.h, n, _tp(boards), _tp(meta), _stream(torch, engine_a.device),
                                         _tp(out["tv"]), _tp(out["dv"]), _tp(summary)))
    s = summary.cpu().tolist()
    out.update({k: v for k, v in zip(COMPARE_SUMMARY[1:], s[1:])}, n=int(s[0]))
    return out
