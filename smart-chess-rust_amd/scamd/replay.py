"""Shuffled trainer-layout minibatches from the compact training tensors, on the GPU (csrc/batch_kernels.hip), and identical
positions merged into one sample each (csrc/merge_kernels.hip)."""
import ctypes as C

import numpy as np

from .binding import MAX_MOVES, PLY_BYTES, _check, _stream, _torch, _tp, lib
from .net import _check_reference_tensors
from .training import _sparse_dtypes_ok

_COMPACT_KEYS = ("boards", "meta", "dist_legal", "legal_idx", "n_legal", "outcome")


def _check_compact_tensors(torch, src):
    """the compact training tensors (layout="reference" with the sparse visit shares) on one GPU -> (device index, rows)"""
    boards, meta = src.get("boards"), src.get("meta")
    if boards is None or meta is None:
        raise ValueError("boards / meta are missing")
    if not boards.is_cuda:
        raise ValueError("boards: a tensor on the GPU is needed")
    device = boards.device.index
    n = _check_reference_tensors(torch, boards, meta, device)
    dl, li, nl, oc = (src.get(k) for k in ("dist_legal", "legal_idx", "n_legal", "outcome"))
    if dl is None or li is None or nl is None:
        raise ValueError('the sparse visit shares (dist_legal + legal_idx + n_legal) are missing: encode with dist="legal" or '
                         'dist="both" -- dense rows are gathered with torch.index_select')
    if oc is None:
        raise ValueError("outcome is missing")
    if not _sparse_dtypes_ok(torch, dl, li, nl) or oc.dtype != torch.float32:
        raise ValueError("dist_legal float32, legal_idx int16, n_legal int32 and outcome float32 are needed")
    dev = torch.device("cuda", device)
    for name, t, shape in (("dist_legal", dl, (n, MAX_MOVES)), ("legal_idx", li, (n, MAX_MOVES)), ("n_legal", nl, (n,)), ("outcome", oc, (n,))):
        if t.device != dev or not t.is_contiguous() or tuple(t.shape) != shape:
            raise ValueError(f"{name}: a contiguous tensor of shape {shape} on cuda:{device} is needed")
    return device, n


def gather_batch_torch(src, rows, mirror=None, n_bad=None):
    """A trainer-layout minibatch from rows of the compact tensors (sc_gather_batch; the reference's DataLoader over ChessDataset
    and _prepare, py/dataset.py:31-87), without leaving the GPU and without a dense dist in memory.
    src: the dict encode_steps_torch(..., layout="reference", dist="legal" | "both") / SelfPlay.training_tensors(...) returns (or
    any dict of boards, meta, dist_legal, legal_idx, n_legal, outcome in that form); rows: int32 / int64 cuda tensor [B] of row
    numbers (a row may repeat); mirror: None, or a cuda tensor [B] (bool / uint8) -- non-zero: the colour-mirrored sample (meta
    of Board::rotate(), outcome negated); n_bad: None, or an int32 cuda tensor [1] that receives the number of samples with bad
    input (row outside the source: all NaN; n_legal outside 0..218 or an action index >= 4672: dist NaN).
    -> (boards float32 [B,112,8,8], meta float32 [B,7], dist float32 [B,4672], outcome float32 [B,1]), enqueued on
    torch.cuda.current_stream()."""
    torch = _torch(cached=True)
    device, n = _check_compact_tensors(torch, src)
    dev = torch.device("cuda", device)
    if rows.dtype not in (torch.int32, torch.int64) or rows.dim() != 1 or rows.device != dev:
        raise ValueError(f"rows: a one-dimensional int32 or int64 tensor on cuda:{device} is needed")
    rows = rows.to(torch.int32).contiguous()
    B = rows.shape[0]
    if mirror is not None:
        if mirror.device != dev or tuple(mirror.shape) != (B,):
            raise ValueError(f"mirror: a tensor of shape ({B},) on cuda:{device} is needed")
        if mirror.dtype == torch.bool:
            mirror = mirror.view(torch.uint8)
        elif mirror.dtype != torch.uint8:
            mirror = (mirror != 0).to(torch.uint8)
        mirror = mirror.contiguous()
    if n_bad is not None and (n_bad.device != dev or n_bad.dtype != torch.int32 or n_bad.numel() < 1):
        raise ValueError(f"n_bad: an int32 tensor on cuda:{device} is needed")
    out = (torch.empty((B, 112, 8, 8), dtype=torch.float32, device=dev), torch.empty((B, 7), dtype=torch.float32, device=dev),
           torch.empty((B, 4672), dtype=torch.float32, device=dev), torch.empty((B, 1), dtype=torch.float32, device=dev))
    _check(lib().sc_gather_batch(device, n, B, _tp(rows), _tp(mirror), _tp(src["boards"]), _tp(src["meta"]), _tp(src["dist_legal"]),
                                 _tp(src["legal_idx"]), _tp(src["n_legal"]), _tp(src["outcome"]), _stream(torch, device),
                                 _tp(out[0]), _tp(out[1]), _tp(out[2]), _tp(out[3]), _tp(n_bad)))
    return out


_merge_ws = {}   # device -> the workspace of merge_positions_torch, a byte tensor kept at the largest size asked for


def _merge_workspace(torch, device, n_in):
    need = C.c_size_t(0)
    _check(lib().sc_merge_positions_workspace(n_in, C.byref(need)))
    ws = _merge_ws.get(device)
    if ws is None or ws.numel() < need.value:
        ws = _merge_ws[device] = torch.empty(need.value, dtype=torch.uint8, device=torch.device("cuda", device))
    return ws


def merge_positions_torch(src, rows=None, key_bits=128):
    """Rows of the compact tensors that are the same sample input -- board bytes, meta, n_legal and legal_idx[:n_legal] -- merged
    into one row each, with the mean visit shares and the mean outcome (sc_merge_positions), without leaving the GPU.
    src: the dict gather_batch_torch takes; rows: None (every row, in order) or an int32 / int64 cuda tensor [n_in] of row numbers
    (position p is row rows[p]; a row may repeat, a row outside the source belongs to no group); key_bits: 128, less only to test
    the byte compare behind the key.
    -> a dict of the same six keys, one row per group (groups ascend with their smallest position), which gather_batch_torch and
    score_torch read as they are, plus count int32 [G] (the group's size), first int32 [G] (its smallest position), group_of int32
    [n_in] (-1: no group), n_bad (rows outside the source, and rows with n_legal outside 0..218, which stay alone) and
    n_key_clash (positions that differed from the head of their key and stay alone: 0 at 128 bits); ply_off / status of src
    are passed on when rows is None.  Enqueued on torch.cuda.current_stream(); the counts are the call's one host read.  The
    workspace is kept per device: calls on one device are expected on one stream at a time."""
    torch = _torch(cached=True)
    device, n = _check_compact_tensors(torch, src)
    dev = torch.device("cuda", device)
    if rows is not None:
        if rows.dtype not in (torch.int32, torch.int64) or rows.dim() != 1 or rows.device != dev:
            raise ValueError(f"rows: a one-dimensional int32 or int64 tensor on cuda:{device} is needed")
        rows = rows.to(torch.int32).contiguous()
    n_in = n if rows is None else int(rows.shape[0])
    ws = _merge_workspace(torch, device, n_in)
    out = {k: torch.empty((n_in,) + tuple(src[k].shape[1:]), dtype=src[k].dtype, device=dev) for k in _COMPACT_KEYS}
    count, first, group_of = (torch.empty(n_in, dtype=torch.int32, device=dev) for _ in range(3))
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    _check(lib().sc_merge_positions(device, n, n_in, _tp(rows), *[_tp(src[k]) for k in _COMPACT_KEYS], int(key_bits), _tp(ws), ws.numel(),
                                    _stream(torch, device), *[_tp(out[k]) for k in _COMPACT_KEYS], _tp(count), _tp(first),
                                    _tp(group_of), _tp(counts)))
    G, n_bad, n_clash, _ = counts.tolist()
    res = {k: v[:G] for k, v in out.items()}
    res.update(count=count[:G], first=first[:G], group_of=group_of, n_bad=n_bad, n_key_clash=n_clash)
    if rows is None:
        res.update({k: src[k] for k in ("ply_off", "status") if k in src})
    return res


def unique_by_ply(tensors):
    """The diversity report of a merge: per ply index, the number of plies and the number of distinct samples among them.
    tensors: group_of (merge_positions_torch's; positions in game order) and ply_off [games + 1] (game g's positions are
    ply_off[g] .. ply_off[g + 1]); optional ply_first [games]: the ply index of each game's first position (default 0).
    -> dict(plies int64 [L], distinct int64 [L]) on the host, L the largest ply index + 1; positions without a group do not count"""
    g = tensors["group_of"]
    g = np.asarray(g.cpu() if hasattr(g, "cpu") else g, np.int64)
    off = np.asarray(tensors["ply_off"], np.int64)
    lens = np.diff(off)
    if int(off[-1]) - int(off[0]) != g.shape[0]:
        raise ValueError("ply_off does not match group_of")
    first = np.asarray(tensors.get("ply_first", np.zeros(len(lens))), np.int64)
    ply = np.concatenate([first[i] + np.arange(n) for i, n in enumerate(lens)]) if len(lens) else np.zeros(0, np.int64)
    L = int(ply.max()) + 1 if ply.size else 0
    keep = g >= 0
    plies = np.bincount(ply[keep], minlength=L)
    pairs = np.unique(np.stack([ply[keep], g[keep]]), axis=1)
    return dict(plies=plies.astype(np.int64), distinct=np.bincount(pairs[0], minlength=L).astype(np.int64))


class ReplayIndex:
    """The bookkeeping of ReplayBuffer, in numpy (no GPU): whole games in a ring of `capacity` rows -- where a new game's plies
    go, which old games leave, which rows a trainer may draw (the reference's start_step rule) and how an epoch is cut."""

    def __init__(self, capacity, start_step=0):
        if capacity <= 0 or start_step < 0:
            raise ValueError("capacity must be positive and start_step non-negative")
        self.capacity, self.start_step = int(capacity), int(start_step)
        self.games = []     # oldest first: (first row, plies); a game's plies are consecutive rows modulo capacity
        self.head = 0       # the next row to be written
        self.used = 0
        self.version = 0    # changes with every add: a running epoch notices that its rows may be gone

    def add_games(self, lengths, status=None):
        """appends the games of one encode result (lengths[g] plies, starting at row sum(lengths[:g]) of it); games with a
        non-zero status or without plies are skipped; the oldest whole games leave until each new one fits.
        -> the copies to make, in order: [(source row, ring row, rows)], none of them wrapping"""
        lengths = [int(x) for x in lengths]
        status = [0] * len(lengths) if status is None else [int(x) for x in status]
        if len(status) != len(lengths):
            raise ValueError("one status per game is needed")
        for n, st in zip(lengths, status):
            if st == 0 and n > self.capacity:
                raise ValueError(f"a game of {n} plies does not fit a buffer of {self.capacity}")
        copies, src = [], 0
        for n, st in zip(lengths, status):
            if st == 0 and n > 0:
                while self.capacity - self.used < n:
                    self.used -= self.games.pop(0)[1]
                self.games.append((self.head, n))
                first = min(n, self.capacity - self.head)
                copies.append((src, self.head, first))
                if first < n:
                    copies.append((src + first, 0, n - first))
                self.head = (self.head + n) % self.capacity
                self.used += n
            src += n
        self.version += 1
        return copies

    def eligible_rows(self):
        """ring rows a trainer may draw, oldest game first: ChessDataset's rule (py/dataset.py:78-80), literally -- a game
        shorter than start_step keeps all its plies, any other its plies start_step: (one of exactly start_step plies: none)"""
        out = []
        for first, n in self.games:
            skip = 0 if n < self.start_step else self.start_step
            out.append((first + np.arange(skip, n, dtype=np.int64)) % self.capacity)
        return np.concatenate(out) if out else np.zeros(0, np.int64)

    @staticmethod
    def epoch_plan(n_eligible, batch_size, drop_last=True):
        """the batches of one epoch as slices [(lo, hi)] of the epoch's order"""
        if batch_size <= 0:
            raise ValueError("batch_size must be positive")
        n_full = n_eligible // batch_size
        plan = [(i * batch_size, (i + 1) * batch_size) for i in range(n_full)]
        if not drop_last and n_eligible % batch_size:
            plan.append((n_full * batch_size, n_eligible))
        return plan

    @staticmethod
    def epoch_seed(seed, epoch):
        """one 63-bit generator seed per (seed, epoch): splitmix64's finaliser over both"""
        z = (int(seed) * 0x9E3779B97F4A7C15 + int(epoch) + 1) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        return (z ^ (z >> 31)) & 0x7FFFFFFFFFFFFFFF


class ReplayBuffer:
    """The reference's DataLoader(ConcatDataset([ChessDataset ...]), batch_size, shuffle=True, drop_last=True) over games kept
    on the GPU in the compact form (8 548 B per ply; allocated once, capacity_plies rows): add() appends the games of an encode
    result and evicts the oldest whole games, batches() yields shuffled trainer-layout minibatches built by sc_gather_batch."""

    def __init__(self, capacity_plies, device=0, start_step=0):
        self.index = ReplayIndex(capacity_plies, start_step)
        self.device = device
        self.store = None
        self._merged = None   # (index version, merged()'s result)

    def __len__(self):
        return int(self.index.eligible_rows().size)

    def _storage(self):
        torch = _torch(cached=True)
        if self.store is None:
            dev, n = torch.device("cuda", self.device), self.index.capacity
            self.store = dict(boards=torch.zeros((n, 8, 8, 112), dtype=torch.int8, device=dev),
                              meta=torch.zeros((n, 7), dtype=torch.int32, device=dev),
                              dist_legal=torch.zeros((n, MAX_MOVES), dtype=torch.float32, device=dev),
                              legal_idx=torch.zeros((n, MAX_MOVES), dtype=torch.int16, device=dev),
                              n_legal=torch.zeros(n, dtype=torch.int32, device=dev),
                              outcome=torch.zeros(n, dtype=torch.float32, device=dev))
            assert sum(t.element_size() * t[0].numel() for t in self.store.values()) == PLY_BYTES
        return torch

    def add(self, tensors):
        """the games of one encode_steps_torch(..., layout="reference", dist="legal" | "both") / SelfPlay.training_tensors
        result (games with status != 0 are skipped).  ValueError for a game longer than the buffer, before anything changes."""
        torch = self._storage()
        device, n = _check_compact_tensors(torch, tensors)
        if device != self.device:
            raise ValueError(f"the tensors are on cuda:{device}, the buffer on cuda:{self.device}")
        ply_off = np.asarray(tensors["ply_off"], np.int64)
        if int(ply_off[-1]) != n:
            raise ValueError("ply_off does not match the number of rows")
        for s, d, k in self.index.add_games(np.diff(ply_off), tensors["status"]):
            for key in _COMPACT_KEYS:
                self.store[key][d:d + k].copy_(tensors[key][s:s + k])

    def merged(self):
        """merge_positions_torch over the eligible rows (oldest game first): one row per distinct sample, targets averaged;
        with ply_off / ply_first of the eligible plies for unique_by_ply.  Computed once, until the next add()."""
        torch = self._storage()
        if self._merged is None or self._merged[0] != self.index.version:
            rows = torch.from_numpy(self.index.eligible_rows()).to(torch.device("cuda", self.device))
            m = merge_positions_torch(self.store, rows)
            skip = [0 if n < self.index.start_step else self.index.start_step for _, n in self.index.games]
            m["ply_off"] = np.concatenate([[0], np.cumsum([n - k for (_, n), k in zip(self.index.games, skip)])]).astype(np.int64)
            m["ply_first"] = np.asarray(skip, np.int64)
            self._merged = (self.index.version, m)
        return self._merged[1]

    def epoch_order(self, seed=0, epoch=0, shuffle=True, mirror=False, unique=False):
        """the rows of one epoch in the order batches() draws them, and their mirror bits: (int32 [E], uint8 [E] or None) on the
        GPU.  The order is torch.randperm on the device from a generator seeded by (seed, epoch); mirror "random" takes one bit
        per sample from the same generator.  unique: the rows are those of merged()."""
        if mirror not in (False, True, "random"):
            raise ValueError('mirror must be False, True or "random"')
        torch = self._storage()
        dev = torch.device("cuda", self.device)
        if unique:
            order = torch.arange(self.merged()["count"].shape[0], dtype=torch.int64, device=dev)
        else:
            order = torch.from_numpy(self.index.eligible_rows()).to(dev)
        E = order.shape[0]
        gen = torch.Generator(device=dev)
        gen.manual_seed(ReplayIndex.epoch_seed(seed, epoch))
        if shuffle:
            order = order[torch.randperm(E, generator=gen, device=dev)]
        if mirror == "random":
            bits = torch.randint(0, 2, (E,), generator=gen, device=dev, dtype=torch.uint8)
        else:
            bits = torch.ones(E, dtype=torch.uint8, device=dev) if mirror else None
        return order.to(torch.int32), bits

    def batches(self, batch_size, seed=0, epoch=0, shuffle=True, drop_last=True, mirror=False, unique=False):
        """one epoch: yields (boards [B,112,8,8], meta [B,7], dist [B,4672], outcome [B,1]), float32 on the GPU, in the order of
        epoch_order(); mirror False / True / "random".  Nothing is copied to the host per batch.  An add() during the epoch ends
        it with a RuntimeError: the rows of the plan may have been evicted.  unique: the epoch runs over merged() -- every distinct
        sample once, with its mean targets; the merge is made once and kept until the next add()."""
        order, bits = self.epoch_order(seed, epoch, shuffle, mirror, unique)
        plan = ReplayIndex.epoch_plan(int(order.shape[0]), batch_size, drop_last)
        return self._epoch(plan, order, bits, self.merged() if unique else self.store)

    def _epoch(self, plan, order, bits, src):
        version = self.index.version
        for lo, hi in plan:
            if self.index.version != version:
                raise RuntimeError("games were added during the epoch: start a new one")
            yield gather_batch_torch(src, order[lo:hi], None if bits is None else bits[lo:hi])
