"""Exact integer k-means over int8 features (include/ivit_cluster.h): `KMeans` owns the int8 centroids, their norms and the three
int64 statistics of an iteration on the device; `step` is one Lloyd iteration — ivit_kmeans_assign and ivit_kmeans_accumulate per
chunk, one ivit_kmeans_update at the end — and `fit` queues `iters` of them with no host round trip.  The seeding (`init`) runs on
the host with exact integer distances.  `KMeansStats` is what ranks combine with ONE integer all-reduce; `contingency`, `purity`
and `nmi` are the two numbers people quote for a clustering against labels.  The numpy statements are
`predict.kmeans_assign_reference`, `kmeans_stats_reference`, `kmeans_update_reference` and `kmeans_reference`.  torch is used for
device memory and streams only."""
import ctypes

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

    def init(self, feat8, method="kmeans++", generator=None, init_rows=65536):
        """seeds the centroids from the rows of feat8 (one tensor or chunks, as `step` takes them), on the HOST, with exact integer
        distances; deterministic for a given `generator` (an np.random.Generator; default np.random.default_rng(0)).
          "sample"    K of the distinct rows, drawn without replacement
          "kmeans++"  D^2 seeding over the distinct rows of at most `init_rows` sampled rows
        Both return K pairwise distinct rows where the sampled rows hold K distinct ones (ValueError otherwise).  Returns self."""
        rows = np.concatenate([c.cpu().numpy() for c in _as_chunks(feat8, self.dim)] + [np.zeros((0, self.dim), np.int8)])
        return self.set_centroids(init_centroids(rows, self.K, method, generator, init_rows))

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
