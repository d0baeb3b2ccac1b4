"""Exact integer k-means over int8 features (include/ivit_cluster.h): `KMeans` owns the int8 centroids, their norms and the three
int64 statistics of an iteration on the device; `step` is one Lloyd iteration — ivit_kmeans_assign and ivit_kmeans_accumulate per
chunk, one ivit_kmeans_update at the end — and `fit` queues `iters` of them with no host round trip.  The seeding (`init`) runs on
the host with exact integer distances or, with where="device", as greedy k-means++ on the device (`seed`, include/ivit_seed.h).
`KMeansStats` is what ranks combine with ONE integer all-reduce; `contingency`, `purity` and `nmi` are the two numbers people quote for a clustering against labels.  The numpy statements are
`predict.kmeans_assign_reference`, `kmeans_stats_reference`, `kmeans_update_reference` and `kmeans_reference`.  torch is used for
device memory and streams only."""
import ctypes
import math

import numpy as np
import torch

from . import _lib

_P = ctypes.c_void_p
MIN_DIM, MAX_DIM, MAX_K = 64, 1024, 16384              # KMEANS_MIN_DIM, KMEANS_MAX_DIM, KMEANS_MAX_K of csrc/ivit_cluster.h


def _ptr(t):
    return None if t is None else _P(t.data_ptr())


def _as_chunks(chunks, dim):
    """one tensor or a list of chunks (device tensors, host tensors, numpy arrays) -> a list of contiguous non-empty int8 tensors"""
    chunks = list(chunks) if isinstance(chunks, (list, tuple)) else [chunks]
    chunks = [c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c)) for c in chunks]
    if any(c.dtype != torch.int8 or c.dim() != 2 or c.shape[1] != dim for c in chunks):
        raise ValueError(f"feat8: int8 [rows, {dim}], or a list of such chunks")
    return [c.contiguous() for c in chunks if c.shape[0]]


class KMeansStats:
    """KMeansStats(K, dim, device): sum int64 [K, dim], count int64 [K], inertia int64 [1], zeroed tensors on `device` — the whole
    state of one iteration's pass over the rows, whatever their number.  Works on any device (the host too: what a gloo rank
    holds)."""

    def __init__(self, K, dim, device="cuda:0"):
        self.K, self.dim, self.device = int(K), int(dim), torch.device(device)
        # one allocation: zeroed with one memset, reduced as one tensor
        self.flat = torch.zeros(self.K * self.dim + self.K + 1, dtype=torch.int64, device=self.device)
        self.sum = self.flat[:self.K * self.dim].view(self.K, self.dim)
        self.count = self.flat[self.K * self.dim:self.K * self.dim + self.K]
        self.inertia = self.flat[self.K * self.dim + self.K:]

    @classmethod
    def from_numpy(cls, total, count, inertia, device="cpu"):
        """the statistics of a numpy triple (`predict.kmeans_stats_reference`) on `device`"""
        total = np.asarray(total)
        out = cls(total.shape[0], total.shape[1], device)
        for t, a in ((out.sum, total), (out.count, count), (out.inertia, np.asarray(inertia).reshape(1))):
            a = np.ascontiguousarray(a, np.int64)
            if tuple(a.shape) != tuple(t.shape):
                raise ValueError(f"shape {a.shape}, expected {tuple(t.shape)}")
            t.copy_(torch.from_numpy(a))
        return out

    def tensors(self):
        return self.sum, self.count, self.inertia

    def all_reduce(self):
        """one all-reduce (sum) of sum, count and inertia over the initialised process group, as ONE int64 tensor; integers: every
        rank ends with the same bits, whatever the order.  gloo reduces host tensors.  Returns self."""
        import torch.distributed as dist
        if not dist.is_initialized():
            raise RuntimeError("KMeansStats.all_reduce needs an initialised process group")
        if dist.get_backend() == "gloo" and self.flat.is_cuda:
            host = self.flat.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.SUM)
            self.flat.copy_(host)
        else:
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM)
        return self

    def numpy(self):
        """(sum, count, inertia) as int64 numpy arrays, the inertia a scalar (synchronises)"""
        s, c, i = (t.cpu().numpy() for t in self.tensors())
        return s, c, np.int64(i[0])

    def zero_(self):
        self.flat.zero_()
        return self


class KMeans:
    """KMeans(K, dim, device): centroids int8 [K, dim], cnorm int32 [K], the statistics of the running iteration (`stats`) and the
    counter `moved` int64 [1], on a HIP device.  `init` or `set_centroids` first; then `step` / `fit` / `assign`."""

    def __init__(self, K, dim, device="cuda:0"):
        K, dim = int(K), int(dim)
        if dim % 64 or not MIN_DIM <= dim <= MAX_DIM:
            raise ValueError(f"dim = {dim}: a multiple of 64 in {MIN_DIM} .. {MAX_DIM}")
        if not 1 <= K <= MAX_K:
            raise ValueError(f"K = {K} outside 1 .. {MAX_K}")
        self.K, self.dim, self.device = K, dim, torch.device(device)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise _lib.IvitError("KMeans needs a HIP device; the product path has no CPU fallback")
        if self.device.index is None:                    # "cuda" names the current device: tensors carry its index
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.centroids = torch.zeros(K, dim, dtype=torch.int8, device=self.device)
        self.cnorm = torch.zeros(K, dtype=torch.int32, device=self.device)
        self.stats = KMeansStats(K, dim, self.device)
        self.moved = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.world = 1                                   # > 1: `step` all-reduces the statistics before the update
        self.h = None
        self._stage = None
        self._out = {}

    # ---- the centroids
    def _handle(self):
        if self.h is None:
            self.h = _lib.Handle(self.device.index, torch.cuda.current_stream(self.device).cuda_stream)
        self.h.set_stream(torch.cuda.current_stream(self.device).cuda_stream)
        return self.h

    def set_centroids(self, cent8):
        """cent8 int8 [K, dim] (numpy, host or device tensor): copied in, the norms recomputed (ivit_kmeans_norms).  Returns self."""
        c = cent8 if isinstance(cent8, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(cent8))
        if c.dtype != torch.int8 or tuple(c.shape) != (self.K, self.dim):
            raise ValueError(f"centroids: int8 [{self.K}, {self.dim}]")
        self.centroids.copy_(c)
        self._handle().call("ivit_kmeans_norms", _ptr(self.centroids), self.K, self.dim, _ptr(self.cnorm))
        return self

    def init(self, feat8, method="kmeans++", generator=None, init_rows=None, where="host", trials=None):
        """seeds the centroids from the rows of feat8 (one tensor or chunks, as `step` takes them) with exact integer distances;
        deterministic for a given `generator` (an np.random.Generator; default np.random.default_rng(0)).
          "sample"    K of the distinct rows, drawn without replacement
          "kmeans++"  D^2 seeding over the distinct rows of at most `init_rows` sampled rows
        where="host" (the default): every row is copied to the host and seeded there (`init_centroids`; init_rows defaults to 65536).
        where="device" ("kmeans++" only): greedy k-means++ by `seed` with `trials` candidates per centre — a device tensor is taken
        as it is, chunks are concatenated on the device, after the host path's row sampling where they hold more than `init_rows`
        (default 2^22) rows.  Both return K pairwise distinct rows where the (sampled) rows hold K distinct ones (ValueError
        otherwise).  Returns self."""
        if where == "host":
            rows = np.concatenate([c.cpu().numpy() for c in _as_chunks(feat8, self.dim)] + [np.zeros((0, self.dim), np.int8)])
            return self.set_centroids(init_centroids(rows, self.K, method, generator, 65536 if init_rows is None else init_rows))
        if where != "device" or method != "kmeans++":
            raise ValueError(f"where = {where!r}, method = {method!r}: 'host', or 'device' with 'kmeans++'")
        rng = np.random.default_rng(0) if generator is None else generator
        if not isinstance(rng, np.random.Generator):
            raise ValueError("generator must be an np.random.Generator")
        chunks = [c.to(self.device) for c in _as_chunks(feat8, self.dim)]
        x = chunks[0] if len(chunks) == 1 else torch.cat(chunks + [torch.zeros(0, self.dim, dtype=torch.int8, device=self.device)])
        init_rows = 1 << 22 if init_rows is None else int(init_rows)
        if x.shape[0] > init_rows:
            keep = np.sort(rng.choice(int(x.shape[0]), size=init_rows, replace=False))
            x = x[torch.from_numpy(keep).to(self.device)]
        out = _seed(self._handle(), x, self.K, trials, rng)
        picked = int(out["picked"].item())
        if picked < self.K:
            raise ValueError(f"{picked} distinct rows among the {x.shape[0]} sampled: fewer than K = {self.K}")
        self.centroids.copy_(out["cent"])
        self.cnorm.copy_(out["cnorm"])
        return self

    # ---- the launches
    def _on_device(self, chunk):
        if chunk.is_cuda:
            return chunk
        if self._stage is None or self._stage.shape[0] < chunk.shape[0]:
            self._stage = torch.empty(int(chunk.shape[0]), self.dim, dtype=torch.int8, device=self.device)
        view = self._stage[:chunk.shape[0]]
        view.copy_(chunk, non_blocking=True)                # stream-ordered behind the last reader
        return view

    def _buffers(self, rows):
        if rows not in self._out:
            if len(self._out) >= 8:
                self._out.pop(next(iter(self._out)))
            self._out[rows] = (torch.empty(rows, dtype=torch.int32, device=self.device), torch.empty(rows, dtype=torch.int32, device=self.device))
        return self._out[rows]

    def assign(self, feat8, copy=False):
        """feat8 int8 device tensor [rows, dim] -> (assign int32 [rows], dist2 int32 [rows]) as `predict.kmeans_assign_reference`
        states them: one ivit_kmeans_assign on the current stream, nothing synchronised.  The results are this object's own
        buffers for this row count: copy=True (or clone) to keep them across calls."""
        if not isinstance(feat8, torch.Tensor) or feat8.dtype != torch.int8 or feat8.dim() != 2 or feat8.shape[1] != self.dim:
            raise ValueError(f"feat8: an int8 tensor [rows, {self.dim}]")
        if feat8.device != self.device or not feat8.is_contiguous():
            raise ValueError(f"feat8: contiguous and on {self.device}, not {feat8.device}")
        rows = int(feat8.shape[0])
        a, d = self._buffers(rows)
        if rows:
            self._handle().call("ivit_kmeans_assign", _ptr(feat8), rows, self.dim, _ptr(self.centroids), _ptr(self.cnorm), self.K, _ptr(a), _ptr(d))
        return (a.clone(), d.clone()) if copy else (a, d)

    def accumulate(self, feat8, assign, dist2=None, splits=0, stats=None):
        """one ivit_kmeans_accumulate of a device chunk into `stats` (default: this object's)"""
        stats = self.stats if stats is None else stats
        if feat8.shape[0]:
            self._handle().call("ivit_kmeans_accumulate", _ptr(feat8), _ptr(assign), _ptr(dist2), int(feat8.shape[0]), self.dim, self.K, int(splits),
                                _ptr(stats.sum), _ptr(stats.count), _ptr(stats.inertia))
        return stats

    def update(self, stats=None):
        """one ivit_kmeans_update from `stats` (default: this object's): centroids and norms rewritten, `moved` added into"""
        stats = self.stats if stats is None else stats
        self._handle().call("ivit_kmeans_update", _ptr(stats.sum), _ptr(stats.count), self.K, self.dim, _ptr(self.centroids), _ptr(self.cnorm),
                            _ptr(self.moved))
        return self

    def step(self, chunks):
        """one Lloyd iteration over one tensor or a list of chunks (host chunks pass through one staging buffer): the statistics
        zeroed, assign and accumulate per chunk, (with world > 1 one all-reduce,) one update.  Nothing synchronises; `stats.inertia`
        then holds the inertia of this iteration's assignment, `moved` has grown by the centroids that changed.  With device
        chunks only, the step is capturable in a graph."""
        self.stats.zero_()
        for c in _as_chunks(chunks, self.dim):
            x = self._on_device(c)
            a, d = self.assign(x)
            self.accumulate(x, a, d)
        if self.world > 1:
            self.stats.all_reduce()
        return self.update()

    def fit(self, chunks, iters=20, tol_moved=0):
        """`iters` Lloyd iterations.  tol_moved == 0: all of them are queued, the inertias are kept on the device and read back ONCE
        at the end.  tol_moved > 0: `moved` is read back after every iteration and the loop ends once an iteration changed fewer
        than tol_moved centroids.  Returns inertia_history, int64 numpy [iterations run]: the inertia of every iteration's
        assignment (not guaranteed monotone: the means are rounded to int8).  `last_moved` holds the number of centroids the
        LAST iteration changed."""
        chunks = _as_chunks(chunks, self.dim)
        history, moved = [], []
        for _ in range(int(iters)):
            self.moved.zero_()
            self.step(chunks)
            history.append(self.stats.inertia.clone())
            moved.append(self.moved.clone())
            if tol_moved > 0 and int(moved[-1].item()) < tol_moved:
                break
        if not history:
            self.last_moved = 0
            return np.zeros(0, np.int64)
        self.last_moved = int(moved[-1].item())
        return torch.cat(history).cpu().numpy()

    def numpy(self):
        """(centroids int8 [K, dim], cnorm int32 [K]) as numpy arrays (synchronises)"""
        return self.centroids.cpu().numpy(), self.cnorm.cpu().numpy()


def _dist2_to(rows32, xx, c):
    """exact squared distances of int32 rows (their squared norms xx) to one int8 row"""
    c = c.astype(np.int32)
    return xx - 2 * (rows32 @ c) + int((c * c).sum())


def init_centroids(rows, K, method="kmeans++", generator=None, init_rows=65536):
    """the host seeding of `KMeans.init`: rows int8 [N, dim] -> int8 [K, dim], K pairwise distinct rows of `rows`"""
    rows = np.asarray(rows)
    assert rows.ndim == 2 and rows.dtype == np.int8
    rng = np.random.default_rng(0) if generator is None else generator
    if not isinstance(rng, np.random.Generator):
        raise ValueError("generator must be an np.random.Generator")
    if method not in ("sample", "kmeans++"):
        raise ValueError(f"method = {method!r}: 'sample' or 'kmeans++'")
    N, K = rows.shape[0], int(K)
    if N > init_rows:
        rows = rows[np.sort(rng.choice(N, size=int(init_rows), replace=False))]
    uniq, first = np.unique(rows, axis=0, return_index=True)       # the distinct rows, each at its first position
    if len(first) < K:
        raise ValueError(f"{len(first)} distinct rows among the {rows.shape[0]} sampled: fewer than K = {K}")
    cand = rows[np.sort(first)]
    if method == "sample":
        return np.ascontiguousarray(cand[np.sort(rng.choice(len(cand), size=K, replace=False))])
    c32 = cand.astype(np.int32)
    xx = (c32 * c32).sum(axis=1).astype(np.int64)
    picked = [int(rng.integers(len(cand)))]
    d = _dist2_to(c32, xx, cand[picked[0]]).astype(np.int64)
    while len(picked) < K:
        total = int(d.sum())                                        # > 0: the candidates are distinct and fewer than K are taken
        t = int(rng.integers(total))                                # an exact integer draw: no float cumsum
        j = int(np.searchsorted(np.cumsum(d), t, side="right"))
        picked.append(j)
        d = np.minimum(d, _dist2_to(c32, xx, cand[j]))
    return np.ascontiguousarray(cand[picked])


# ---------------------------------------------------------------- the device seeding (include/ivit_seed.h)
MAX_TRIALS = 32                                        # SEED_MAX_TRIALS of csrc/ivit_seed.h


def default_trials(K):
    """2 + floor(ln K), scikit-learn's number of candidates per centre, capped at the 32 a launch evaluates at once"""
    return min(MAX_TRIALS, 2 + int(math.floor(math.log(int(K)))))


def seed_draws(rows, K, trials, generator):
    """the random input of a seeding: (first, draws uint64 [K, trials]) from the generator, in this order"""
    first = int(generator.integers(int(rows)))
    return first, generator.integers(0, 2 ** 64, size=(int(K), int(trials)), dtype=np.uint64)


def _seed(handle, feat8, K, trials, rng):
    """one ivit_kmeans_seed on the handle's stream over a contiguous int8 device tensor: every output of the entry, on the device"""
    if not isinstance(feat8, torch.Tensor) or feat8.dtype != torch.int8 or feat8.dim() != 2 or not feat8.is_cuda or not feat8.is_contiguous():
        raise ValueError("feat8: a contiguous int8 device tensor [rows, dim]")
    rows, dim, K = int(feat8.shape[0]), int(feat8.shape[1]), int(K)
    trials = default_trials(K) if trials is None else int(trials)
    if rows < 1:
        raise ValueError("feat8 holds no row")
    first, draws = seed_draws(rows, K, trials, rng)
    nbytes = ctypes.c_size_t(0)
    st = handle.lib.ivit_kmeans_seed_workspace_bytes(rows, dim, trials, ctypes.byref(nbytes))
    if st != 0:
        raise _lib.IvitError(f"ivit_kmeans_seed_workspace_bytes(rows={rows}, dim={dim}, trials={trials}): {handle.lib.ivit_status_string(st).decode()}")
    dev = feat8.device
    out = {"cent": torch.empty(K, dim, dtype=torch.int8, device=dev), "cnorm": torch.empty(K, dtype=torch.int32, device=dev),
           "idx": torch.empty(K, dtype=torch.int32, device=dev), "potential": torch.empty(K, dtype=torch.int64, device=dev),
           "picked": torch.empty(1, dtype=torch.int32, device=dev)}
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    d = torch.from_numpy(draws.view(np.int64)).to(dev)                  # the same 64 bits
    handle.call("ivit_kmeans_seed", _ptr(feat8), rows, dim, K, trials, first, _ptr(d), _ptr(ws), nbytes.value, _ptr(out["cent"]),
                _ptr(out["cnorm"]), _ptr(out["idx"]), _ptr(out["potential"]), _ptr(out["picked"]))
    for t in (ws, d):
        t.record_stream(torch.cuda.current_stream(dev))                 # freed here, read by the queued launches
    return out


def seed(feat8, K, trials=None, generator=None):
    """greedy k-means++ seeding of K centres from the rows of feat8 (a contiguous int8 device tensor [rows, dim]) ON THE DEVICE, as
    `predict.kmeans_seed_reference` states it: `trials` candidates per centre (None: `default_trials(K)`; 1 is plain k-means++),
    `first` and the draws from `generator` (an np.random.Generator; default np.random.default_rng(0)) by `seed_draws`.  Queued on the
    current stream, nothing synchronised.  Returns (idx int32 [K], cent8 int8 [K, dim], potential int64 [K]) on the device; where
    the rows hold fewer than K distinct ones, idx is -1 from the first centre that could not be drawn."""
    rng = np.random.default_rng(0) if generator is None else generator
    if not isinstance(rng, np.random.Generator):
        raise ValueError("generator must be an np.random.Generator")
    if not isinstance(feat8, torch.Tensor) or not feat8.is_cuda:
        raise ValueError("feat8: a contiguous int8 device tensor [rows, dim]")
    h = _lib.Handle(feat8.device.index, torch.cuda.current_stream(feat8.device).cuda_stream)
    out = _seed(h, feat8, K, trials, rng)
    return out["idx"], out["cent"], out["potential"]


# ---------------------------------------------------------------- a clustering against labels
def contingency(assign, labels, K, C):
    """assign integer tensor [rows], labels integer tensor [rows] on one device -> int64 [K, C]: table[j, c] = rows of cluster j with
    label c (one bincount on that device); a row whose cluster or label is out of range is left out"""
    a, l = torch.as_tensor(assign).reshape(-1).to(torch.int64), torch.as_tensor(labels).reshape(-1).to(torch.int64)
    l = l.to(a.device)
    assert a.shape == l.shape
    K, C = int(K), int(C)
    keep = (a >= 0) & (a < K) & (l >= 0) & (l < C)
    return torch.bincount(a[keep] * C + l[keep], minlength=K * C).reshape(K, C)


def contingency_reference(assign, labels, K, C):
    a, l = np.asarray(assign).astype(np.int64).reshape(-1), np.asarray(labels).astype(np.int64).reshape(-1)
    table = np.zeros((int(K), int(C)), np.int64)
    keep = (a >= 0) & (a < K) & (l >= 0) & (l < C)
    np.add.at(table, (a[keep], l[keep]), 1)
    return table


def purity(table):
    """table [K, C] -> sum_j max_c table[j, c] / n in float64 (nan for an empty table)"""
    t = np.asarray(table.cpu() if isinstance(table, torch.Tensor) else table).astype(np.float64)
    n = t.sum()
    return float(t.max(axis=1).sum() / n) if n > 0 else float("nan")


def nmi(table):
    """table [K, C] -> normalised mutual information I(cluster; label) / ((H(cluster) + H(label)) / 2) in float64, natural
    logarithms, 0 log 0 = 0; 1.0 where both entropies are 0 (one cluster, one label); nan for an empty table"""
    t = np.asarray(table.cpu() if isinstance(table, torch.Tensor) else table).astype(np.float64)
    n = t.sum()
    if not n > 0:
        return float("nan")
    p, pa, pb = t / n, t.sum(axis=1) / n, t.sum(axis=0) / n

    def H(q):
        q = q[q > 0]
        return float(-(q * np.log(q)).sum())
    outer = np.outer(pa, pb)
    nz = p > 0
    mi = float((p[nz] * np.log(p[nz] / outer[nz])).sum())
    den = (H(pa) + H(pb)) / 2
    return mi / den if den > 0 else 1.0


# ---------------------------------------------------------------- density clustering (include/ivit_density.h)
NONE = 2 ** 31 - 1                                     # DENSITY_NONE of csrc/ivit_density.h: the label of a row that is not core


def dbscan(feat8, threshold, min_pts, cosine=True, check_every=4, splits=0):
    """DBSCAN over the rows of feat8 (a contiguous int8 device tensor [rows, dim]) ON THE DEVICE, as `predict.dbscan_reference`
    states it, with the rows' inverse norms (ivit_gallery_inv_norms) as the weight for cosine=True and none for the exact integer
    dot product.  The order of work: ivit_density_degree, ivit_density_init, then batches of `check_every` ivit_density_sweep with
    ONE read of `changed` per batch (the only synchronisations) until a batch ends on 0, then ivit_density_border.  A sweep after
    convergence skips every tile, so a larger check_every costs little; the labels depend neither on it nor on `splits`.  Memory is
    O(rows): no pair list, no [rows, rows] matrix.  Returns (label int32 [rows]: the smallest row of the cluster, -1 for noise; core
    bool [rows]; degree int32 [rows]; sweeps: the number of sweeps queued)."""
    if not isinstance(feat8, torch.Tensor) or feat8.dtype != torch.int8 or feat8.dim() != 2 or not feat8.is_cuda or not feat8.is_contiguous():
        raise ValueError("feat8: a contiguous int8 device tensor [rows, dim]")
    rows, dim, dev = int(feat8.shape[0]), int(feat8.shape[1]), feat8.device
    if rows < 1:
        raise ValueError("feat8 holds no row")
    if not np.isfinite(np.float32(threshold)):
        raise ValueError("threshold must be finite")
    if int(min_pts) < 1 or int(check_every) < 1:
        raise ValueError("min_pts and check_every must be at least 1")
    h = _lib.Handle(dev.index, torch.cuda.current_stream(dev).cuda_stream)
    n = ctypes.c_size_t()
    h.call("ivit_density_workspace_bytes", rows, dim, int(splits), ctypes.byref(n))
    new = lambda dt, *shape: torch.empty(*shape, dtype=dt, device=dev)      # noqa: E731
    ws = new(torch.uint8, n.value)
    weight = None
    if cosine:
        weight = new(torch.float32, rows)
        h.call("ivit_gallery_inv_norms", _ptr(feat8), rows, dim, _ptr(weight))
    scan = (_ptr(feat8), rows, dim, _ptr(weight), float(threshold), int(splits), _ptr(ws), n.value)
    words = ((rows + 31) // 32 + 63) // 64
    degree, out, changed = new(torch.int32, rows), new(torch.int32, rows), new(torch.int32, 1)
    label, dirty = [new(torch.int32, rows), new(torch.int32, rows)], [new(torch.int64, words), new(torch.int64, words)]
    h.call("ivit_density_degree", *scan, _ptr(degree))
    h.call("ivit_density_init", _ptr(degree), rows, int(min_pts), _ptr(label[0]), _ptr(dirty[0]))
    sweeps = 0
    while True:
        for _ in range(int(check_every)):
            a, b = sweeps & 1, ~sweeps & 1
            h.call("ivit_density_sweep", *scan, _ptr(label[a]), _ptr(dirty[a]), _ptr(label[b]), _ptr(dirty[b]), _ptr(changed))
            sweeps += 1
        if int(changed.item()) == 0:                                    # the one read of a batch
            break
        if sweeps > rows + int(check_every):
            raise _lib.IvitError("ivit_density_sweep did not converge: labels only fall, so this cannot happen")
    h.call("ivit_density_border", *scan, _ptr(label[sweeps & 1]), _ptr(out))
    return out, label[sweeps & 1] != NONE, degree, sweeps


def compact_labels(label):
    """label integer tensor [rows] (`dbscan`: a cluster is named by its smallest row) -> (int32 [rows] on the same device with the
    clusters numbered 0 .. n_clusters - 1 in ascending order of their label, noise still -1; n_clusters)"""
    label = torch.as_tensor(label).reshape(-1)
    names = torch.unique(label[label >= 0])                            # sorted
    compact = torch.where(label >= 0, torch.searchsorted(names, label.clamp(min=0)), torch.full_like(label, -1))
    return compact.to(torch.int32), int(names.shape[0])


# ---------------------------------------------------------------- single-linkage hierarchy (include/ivit_linkage.h)
class Linkage:
    """The spanning forest of a single-linkage hierarchy over `rows` rows: u < v int32 [E] and val float32 [E], the edges in the edge
    order of include/ivit_linkage.h (val descending, then u, then v ascending), as tensors (on the device from `single_linkage`; numpy
    arrays are taken as host tensors); `rounds`: the Borůvka rounds that merged something."""

    def __init__(self, u, v, val, rows, rounds=0):
        self.u, self.v, self.val = (torch.as_tensor(t) for t in (u, v, val))
        self.rows, self.rounds = int(rows), int(rounds)

    def _groups(self, keep):
        from .search import duplicate_groups
        return duplicate_groups(torch.stack([self.u[keep], self.v[keep]], 1), self.rows)

    def cut(self, threshold):
        """int64 [rows] on the host: for every row the smallest row it is connected to through edges with val >= threshold — the
        components of the graph v >= threshold, `search.duplicate_groups` of `search.duplicates` at that threshold, for ANY threshold at
        or above the floor the forest was built with."""
        return self._groups(self.val >= torch.tensor(float(np.float32(threshold)), dtype=torch.float32, device=self.val.device))

    def cut_k(self, n_clusters):
        """the same after removing the n_clusters - 1 last edges in the edge order: n_clusters groups of a tree (a forest built with a
        floor starts from its own components)"""
        if int(n_clusters) < 1:
            raise ValueError("n_clusters must be at least 1")
        return self._groups(slice(0, max(0, self.u.shape[0] - (int(n_clusters) - 1))))

    def matrix(self):
        """float64 [E, 4] on the host, in plain numpy: the linkage matrix in SciPy's convention — step s joins clusters Z[s, 0] < Z[s, 1]
        (a row, or rows + t for the cluster step t made) at distance Z[s, 2] = -val into one of Z[s, 3] rows — the edges taken in the
        edge order."""
        u, v, val = (t.cpu().numpy() for t in (self.u, self.v, self.val))
        root, name, size = list(range(self.rows)), list(range(self.rows)), [1] * self.rows
        Z = np.zeros((len(u), 4), np.float64)

        def find(a):
            while root[a] != a:
                root[a] = root[root[a]]
                a = root[a]
            return a
        for s in range(len(u)):
            a, b = find(int(u[s])), find(int(v[s]))
            Z[s] = min(name[a], name[b]), max(name[a], name[b]), -np.float64(val[s]), size[a] + size[b]
            root[b], name[a], size[a] = a, self.rows + s, size[a] + size[b]
        return Z

    def condense(self, min_cluster_size, floor=None):
        """the `CondensedTree` of this forest as `predict.hdbscan_labels_reference` states it, in plain numpy / Python on the host: Kruskal
        over GROUPS of equal value (the levels, so no tie order enters), then the walk from the roots.  `floor`: the floor the forest was
        built with (the roots' birth); None: the lowest edge value."""
        return CondensedTree(self, min_cluster_size, floor)


class CondensedTree:
    """The condensed tree of HDBSCAN over a `Linkage` (the forest of the mutual-reachability values): cluster c is number rows + c.
      parent, child, lam, size   int64, int64, float32, int64 [entries]: `child` (a row, size 1, or a cluster with `size` rows) leaves or
                                 is born out of cluster `parent` at level `lam`
      birth, name                float32, int64 [clusters]: the level a cluster is born at and its smallest row
      up                         int64 [clusters]: the parent cluster's number, -1 for a root
      stability                  float64 [clusters]: math.fsum of float64(lam) - float64(birth) over the rows that leave the cluster,
                                 one term per row, those that enter a child cluster included
    Levels, not a binary merge order, define it: the edges of one value are united together and the clusters they join become the
    children of ONE node."""

    def __init__(self, tree, min_cluster_size, floor=None):
        mcs, rows = int(min_cluster_size), tree.rows
        if mcs < 2:
            raise ValueError("min_cluster_size must be at least 2")
        u, v, val = (t.cpu().numpy() for t in (tree.u, tree.v, tree.val))
        self.rows, self.min_cluster_size = rows, mcs
        # the level dendrogram: node n < rows is row n; a later node holds the nodes one level joined
        root, node = list(range(rows)), list(range(rows))
        kids, level, size, low = [None] * rows, [None] * rows, [1] * rows, list(range(rows))

        def find(a):
            while root[a] != a:
                root[a] = root[root[a]]
                a = root[a]
            return a
        s = 0
        while s < len(u):
            e = s
            while e < len(u) and val[e] == val[s]:
                e += 1
            old = sorted({find(int(a)) for a in u[s:e]} | {find(int(a)) for a in v[s:e]})
            joined = [node[a] for a in old]
            for a, b in zip(u[s:e].tolist(), v[s:e].tolist()):
                a, b = find(a), find(b)
                root[max(a, b)] = min(a, b)
            groups = {}
            for a, n in zip(old, joined):
                groups.setdefault(find(a), []).append(n)
            for a, ns in groups.items():
                node[a] = len(kids)
                kids.append(ns)
                level.append(val[s])
                size.append(sum(size[n] for n in ns))
                low.append(min(low[n] for n in ns))
            s = e

        def leaves(n):
            out, todo = [], [n]
            while todo:
                n = todo.pop()
                if n < rows:
                    out.append(n)
                else:
                    todo.extend(kids[n])
            return out
        base = np.float32(floor) if floor is not None else (val[-1] if len(val) else np.float32(0))
        parent, child, lam, csize, birth, name, up = [], [], [], [], [], [], []
        todo = []
        for a in sorted({find(q) for q in range(rows)}):
            if size[node[a]] >= mcs:
                todo.append((len(birth), node[a]))
                birth.append(base), name.append(low[node[a]]), up.append(-1)
        while todo:
            c, n = todo.pop()
            while True:
                big = [k for k in kids[n] if size[k] >= mcs]
                for k in kids[n]:
                    if size[k] < mcs or len(big) == 0:
                        for q in leaves(k):
                            parent.append(rows + c), child.append(q), lam.append(level[n]), csize.append(1)
                if len(big) != 1:
                    break
                n = big[0]
            if len(big) >= 2:
                for k in big:
                    parent.append(rows + c), child.append(rows + len(birth)), lam.append(level[n]), csize.append(size[k])
                    todo.append((len(birth), k))
                    birth.append(level[n]), name.append(low[k]), up.append(c)
        self.parent, self.child, self.size = (np.asarray(a, np.int64) for a in (parent, child, csize))
        self.lam, self.birth = np.asarray(lam, np.float32), np.asarray(birth, np.float32)
        self.name, self.up = np.asarray(name, np.int64), np.asarray(up, np.int64)
        terms = [[] for _ in birth]
        for p, l, n in zip(parent, lam, csize):
            terms[p - rows] += [float(np.float64(l) - np.float64(birth[p - rows]))] * n
        self.stability = np.asarray([math.fsum(t) for t in terms], np.float64)

    def select(self, method="eom", allow_single_cluster=False):
        """int32 [rows] on the host: the smallest row of the selected cluster a row belongs to, -1 for noise.  "eom": bottom-up, a leaf
        is selected, an inner cluster is selected and its descendants unselected unless the fsum of its children's subtree totals is
        STRICTLY greater than its stability; "leaf": the leaves.  Where there is exactly one root it is selectable only with
        allow_single_cluster."""
        if method not in ("eom", "leaf"):
            raise ValueError(f"method = {method!r}: 'eom' or 'leaf'")
        n = len(self.birth)
        children = [[] for _ in range(n)]
        for c in range(n):
            if self.up[c] >= 0:
                children[self.up[c]].append(c)
        single = int((self.up < 0).sum()) == 1 and not allow_single_cluster
        total, chosen = [0.0] * n, [False] * n
        for c in range(n - 1, -1, -1):                                  # a child's number is above its parent's
            selectable = not (single and self.up[c] < 0)
            below = math.fsum(total[k] for k in children[c])
            if not children[c]:
                chosen[c], total[c] = selectable, float(self.stability[c]) if selectable else 0.0
            elif method == "leaf" or not selectable or below > self.stability[c]:
                total[c] = below
            else:
                chosen[c], total[c] = True, float(self.stability[c])
        owner = np.full(n, -1, np.int64)                                # the selected cluster at or above each cluster, top-down
        for c in range(n):
            owner[c] = owner[self.up[c]] if self.up[c] >= 0 and owner[self.up[c]] >= 0 else (self.name[c] if chosen[c] else -1)
        label = np.full(self.rows, -1, np.int32)
        is_row = self.child < self.rows
        label[self.child[is_row]] = owner[self.parent[is_row] - self.rows]
        return label


def _hdbscan_setup(feat8, cosine, splits):
    if not isinstance(feat8, torch.Tensor) or feat8.dtype != torch.int8 or feat8.dim() != 2 or not feat8.is_cuda or not feat8.is_contiguous():
        raise ValueError("feat8: a contiguous int8 device tensor [rows, dim]")
    rows, dim, dev = int(feat8.shape[0]), int(feat8.shape[1]), feat8.device
    if rows < 1:
        raise ValueError("feat8 holds no row")
    h = _lib.Handle(dev.index, torch.cuda.current_stream(dev).cuda_stream)
    weight = None
    if cosine:
        weight = torch.empty(rows, dtype=torch.float32, device=dev)
        h.call("ivit_gallery_inv_norms", _ptr(feat8), rows, dim, _ptr(weight))
    return h, rows, dim, dev, weight


def _kth(h, feat8, rows, dim, weight, k, splits):
    """ivit_kth_similarity as a self-join -> (kth float32 [rows], above int64 [rows])"""
    n = ctypes.c_size_t()
    h.call("ivit_kth_workspace_bytes", rows, rows, dim, int(splits), 1, ctypes.byref(n))
    new = lambda dt, m: torch.empty(m, dtype=dt, device=feat8.device)      # noqa: E731
    ws, kth, above = new(torch.uint8, n.value) if n.value else None, new(torch.float32, rows), new(torch.int64, rows)
    h.call("ivit_kth_similarity", _ptr(feat8), rows, _ptr(feat8), rows, dim, _ptr(weight), None, int(k), 1, int(splits), _ptr(ws), n.value,
           _ptr(kth), _ptr(above))
    if ws is not None:
        ws.record_stream(torch.cuda.current_stream(feat8.device))       # freed here, read by the queued launches
    return kth, above


def kth_similarity(feat8, k, cosine=True, splits=0):
    """(kth float32 [rows], above int64 [rows]) on the device: for every row of feat8 (a contiguous int8 device tensor [rows, dim]) its
    k-th largest value among all rows, itself included and equal values with their multiplicity, and the number of rows strictly above
    it, as `predict.kth_reference(feat8, feat8, weight, None, k, self_join=True)` states them (ivit_kth_similarity: an exact radix
    select, k in 1 .. rows).  For k <= 64 kth is `core_similarity`'s, bit for bit.  Queued on the current stream, nothing
    synchronised; nothing depends on `splits`."""
    h, rows, dim, _, weight = _hdbscan_setup(feat8, cosine, splits)
    return _kth(h, feat8, rows, dim, weight, k, splits)


def _core(h, feat8, rows, dim, weight, min_pts, splits):
    if int(min_pts) > 64:                                               # beyond the candidate lists of ivit_core_similarity: the radix select
        return _kth(h, feat8, rows, dim, weight, min_pts, splits)[0]
    n = ctypes.c_size_t()
    h.call("ivit_core_workspace_bytes", rows, dim, int(min_pts), int(splits), ctypes.byref(n))
    ws, core = torch.empty(n.value, dtype=torch.uint8, device=feat8.device), torch.empty(rows, dtype=torch.float32, device=feat8.device)
    h.call("ivit_core_similarity", _ptr(feat8), rows, dim, _ptr(weight), int(min_pts), int(splits), _ptr(ws), n.value, _ptr(core))
    ws.record_stream(torch.cuda.current_stream(feat8.device))           # freed here, read by the queued launches
    return core


def core_similarity(feat8, min_pts, cosine=True, splits=0):
    """float32 [rows] on the device: for every row of feat8 (a contiguous int8 device tensor [rows, dim]) its min_pts-th largest value
    among all rows, itself included and equal values with their multiplicity, as `predict.mutual_reachability_reference` states it
    (ivit_core_similarity for min_pts in 1 .. min(rows, 64); above 64, up to rows, ivit_kth_similarity, the same values by radix
    select as `predict.kth_reference` states them).  `degree >= min_pts` of `dbscan` at a threshold t is `core >= t`.  Queued
    on the current stream, nothing synchronised."""
    h, rows, dim, _, weight = _hdbscan_setup(feat8, cosine, splits)
    return _core(h, feat8, rows, dim, weight, min_pts, splits)


def hdbscan(feat8, min_cluster_size=5, min_pts=None, cosine=True, floor=None, selection="eom", allow_single_cluster=False, splits=0, check_every=1):
    """HDBSCAN over the rows of feat8 (a contiguous int8 device tensor [rows, dim]) as `predict.hdbscan_reference` and
    `predict.hdbscan_labels_reference` state it; min_pts defaults to min_cluster_size (clipped to the rows and to 64; an EXPLICIT
    min_pts may go up to the rows: above 64 the core similarities come from ivit_kth_similarity).  ON THE DEVICE:
    ivit_core_similarity, ivit_linkage_init, then batches of `check_every` ivit_reach_round with one read of `state` per batch, as
    `single_linkage`; the edges are sorted into the edge order there too.  ON THE HOST over those rows - 1 edges: `Linkage.condense`
    and `CondensedTree.select`.  Memory is O(rows); nothing depends on `splits` or `check_every`.  Returns (label int32 [rows] on the
    device: the smallest row of the row's cluster, -1 for noise — `compact_labels` numbers them; core float32 [rows]; tree: the
    `Linkage` of the mutual-reachability forest; condensed: the `CondensedTree`)."""
    h, rows, dim, dev, weight = _hdbscan_setup(feat8, cosine, splits)
    min_pts = min(int(min_cluster_size), rows, 64) if min_pts is None else int(min_pts)
    core = _core(h, feat8, rows, dim, weight, min_pts, splits)
    tree = _forest(h, feat8, rows, dim, weight, floor, splits, check_every, core)
    condensed = tree.condense(min_cluster_size, floor)
    return torch.from_numpy(condensed.select(selection, allow_single_cluster)).to(dev), core, tree, condensed


def single_linkage(feat8, cosine=True, floor=None, splits=0, check_every=1):
    """The single-linkage hierarchy of the rows of feat8 (a contiguous int8 device tensor [rows, dim]) ON THE DEVICE, as
    `predict.linkage_reference` states it, with the rows' inverse norms (ivit_gallery_inv_norms) as the weight for cosine=True and none
    for the exact integer dot product; floor None is -infinity (a tree of rows - 1 edges).  ivit_linkage_init, then batches of
    `check_every` ivit_linkage_round with ONE read of `state` per batch (the only synchronisations) until it reports merged == 0 or one
    component; a round past the end leaves at once.  The edges depend neither on check_every nor on `splits`.  Memory is O(rows).  The
    empty slots are dropped and the edges sorted into the edge order with stable torch sorts.  Returns a `Linkage`."""
    if not isinstance(feat8, torch.Tensor) or feat8.dtype != torch.int8 or feat8.dim() != 2 or not feat8.is_cuda or not feat8.is_contiguous():
        raise ValueError("feat8: a contiguous int8 device tensor [rows, dim]")
    rows, dim, dev = int(feat8.shape[0]), int(feat8.shape[1]), feat8.device
    if rows < 1:
        raise ValueError("feat8 holds no row")
    h = _lib.Handle(dev.index, torch.cuda.current_stream(dev).cuda_stream)
    weight = None
    if cosine:
        weight = torch.empty(rows, dtype=torch.float32, device=dev)
        h.call("ivit_gallery_inv_norms", _ptr(feat8), rows, dim, _ptr(weight))
    return _forest(h, feat8, rows, dim, weight, floor, splits, check_every)


def _forest(h, feat8, rows, dim, weight, floor, splits, check_every, core=None):
    """the rounds of `single_linkage` (core None: ivit_linkage_round) or of `hdbscan` (ivit_reach_round over `core`) -> a `Linkage`"""
    dev = feat8.device
    floor = float("-inf") if floor is None else float(np.float32(floor))
    if math.isnan(floor):
        raise ValueError("floor must not be NaN")
    if int(check_every) < 1:
        raise ValueError("check_every must be at least 1")
    n = ctypes.c_size_t()
    h.call("ivit_linkage_workspace_bytes", rows, dim, int(splits), ctypes.byref(n))
    new = lambda dt, *shape: torch.empty(*shape, dtype=dt, device=dev)      # noqa: E731
    ws = new(torch.uint8, n.value)
    comp, done, state = new(torch.int32, rows), new(torch.uint8, rows), new(torch.int32, 4)
    u, v, val = new(torch.int32, rows), new(torch.int32, rows), new(torch.float32, rows)
    run = tuple(_ptr(t) for t in (comp, done, u, v, val, state))
    h.call("ivit_linkage_init", rows, *run)
    while True:
        for _ in range(int(check_every)):
            if core is None:
                h.call("ivit_linkage_round", _ptr(feat8), rows, dim, _ptr(weight), floor, int(splits), _ptr(ws), n.value, *run)
            else:
                h.call("ivit_reach_round", _ptr(feat8), rows, dim, _ptr(weight), _ptr(core), floor, int(splits), _ptr(ws), n.value, *run)
        components, merged, rounds, _ = state.tolist()                  # the one read of a batch
        if merged == 0 or components == 1:
            break
    keep = u >= 0
    edges = [u[keep], v[keep], val[keep]]
    for key, descending in ((1, False), (0, False), (2, True)):         # v, then u, then val: the last sort is the first criterion
        order = torch.sort(edges[key], stable=True, descending=descending)[1]
        edges = [t[order] for t in edges]
    return Linkage(*edges, rows, rounds)
