"""Gallery search over the engines' int8 features (include/ivit_search.h): `Gallery` holds the rows (and, for cosine, their inverse
norms) and finds every query's k nearest through `ivit_search_topk` — the gallery streamed once, the scores never written — chunk by
chunk with `ivit_search_merge` behind when it was given in pieces; `knn_classify` is the weighted vote of the usual k-NN protocol
for a frozen backbone on the small [B, k] results, `knn_reference` its numpy statement.  The numpy statements of the search itself
are `predict.search_reference` and `predict.inv_norms_reference`.  `Gallery.within` is the threshold form (include/ivit_range.h: all
rows with a score >= threshold, in CSR form, `predict.range_reference` its numpy statement), `duplicates` / `cross_matches` the
self-join and the join of two sets built on it, `duplicate_groups` the connected components of the pairs (host).  torch is used for
device memory and streams, for the vote and for laying the chunks' rows side by side."""
import ctypes

import numpy as np
import torch

from . import _lib
from .native import ShapeCache

_P = ctypes.c_void_p
MAX_K = 64           # SEARCH_MAX_K of csrc/ivit_search.h


def _ptr(t):
    return None if t is None else _P(t.data_ptr())


def query_inv_norms(feat8):
    """int8 device tensor [B, dim] -> float64 [B]: 1 / |q|, 0 for a row of zeros (what turns a cosine gallery's values into cosines)"""
    ss = (feat8.to(torch.int64) ** 2).sum(1).to(torch.float64)
    return torch.where(ss > 0, 1.0 / torch.sqrt(torch.where(ss > 0, ss, torch.ones_like(ss))), torch.zeros_like(ss))


class Gallery:
    """Gallery(feat8, labels=None, cosine=True, chunk_rows=None): int8 rows [N, dim] to search.

    feat8       an int8 device tensor [N, dim] (`predict.embed8`), or a list of chunks [n_i, dim]: device tensors, host tensors or
                numpy arrays.  A host chunk stays on the host and passes through ONE staging buffer on the device at every search —
                the way to a gallery larger than device memory.  chunk_rows cuts a device tensor into chunks of that many rows.
    labels      integers [N] (any form torch.as_tensor takes), or None: kept as an int64 device tensor for `knn_classify`.
    cosine      True: the rows' inverse norms are computed once (ivit_gallery_inv_norms) and weigh every score, so a query's
                neighbours come in cosine order; False: in the order of the exact integer dot product.
    One chunk is one ivit_search_topk; several are one each, with the chunk's first row as index_base, laid side by side and
    combined by ONE ivit_search_merge: the same (idx, val) as the one-piece search, bit for bit."""

    def __init__(self, feat8, labels=None, cosine=True, chunk_rows=None, num_classes=None, device=None):
        chunks = list(feat8) if isinstance(feat8, (list, tuple)) else [feat8]
        chunks = [c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c)) for c in chunks]
        if not chunks or any(c.dtype != torch.int8 or c.dim() != 2 or c.shape[1] != chunks[0].shape[1] for c in chunks):
            raise ValueError("feat8: int8 [N, dim], or a non-empty list of such chunks of one dim")
        on_device = [c for c in chunks if c.is_cuda]
        self.device = torch.device(device) if device is not None else (on_device[0].device if on_device else torch.device("cuda", torch.cuda.current_device()))
        if not torch.cuda.is_available():
            raise _lib.IvitError("Gallery needs a HIP device; the product path has no CPU fallback")
        if chunk_rows is not None:
            if int(chunk_rows) < 1:
                raise ValueError("chunk_rows must be positive")
            chunks = [part for c in chunks for part in (c.split(int(chunk_rows)) if c.shape[0] else [c])]
        chunks = [c.contiguous() for c in chunks if c.shape[0]]
        if not chunks:
            raise ValueError("feat8 has no rows")
        self.chunks, self.dim, self.cosine = chunks, int(chunks[0].shape[1]), bool(cosine)
        self.starts = [0]
        for c in chunks:
            self.starts.append(self.starts[-1] + int(c.shape[0]))
        self.rows = self.starts[-1]
        self.labels = None if labels is None else torch.as_tensor(labels).to(device=self.device, dtype=torch.int64).reshape(-1)
        if self.labels is not None and self.labels.shape[0] != self.rows:
            raise ValueError(f"{self.labels.shape[0]} labels for {self.rows} rows")
        self.num_classes = int(num_classes) if num_classes is not None else (int(self.labels.max()) + 1 if self.labels is not None else None)
        torch.cuda.set_device(self.device)
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.h = _lib.Handle(dev_index, torch.cuda.current_stream(self.device).cuda_stream)
        host_rows = max([int(c.shape[0]) for c in chunks if not c.is_cuda], default=0)
        self._stage = torch.empty(host_rows, self.dim, dtype=torch.int8, device=self.device) if host_rows else None
        self.inv_norm = None
        if self.cosine:
            self.inv_norm = torch.empty(self.rows, dtype=torch.float32, device=self.device)
            for c, s in zip(chunks, self.starts):
                d = self._on_device(c)
                self.h.call("ivit_gallery_inv_norms", _ptr(d), int(c.shape[0]), self.dim, _P(self.inv_norm.data_ptr() + 4 * s))
        self._bufs = ShapeCache(self._make_buffers)        # (nq, k) -> workspace, candidates, outputs: the gallery's own

    def _on_device(self, chunk):
        """the chunk where the kernels read it: itself, or its copy in the staging buffer (stream-ordered behind the last reader)"""
        if chunk.is_cuda:
            return chunk
        view = self._stage[:chunk.shape[0]]
        view.copy_(chunk, non_blocking=True)
        return view

    def _make_buffers(self, nq, k):
        need, n = 0, ctypes.c_size_t()
        ks = [min(k, int(c.shape[0])) for c in self.chunks]
        for c, kc in zip(self.chunks, ks):
            self.h.call("ivit_search_workspace_bytes", nq, int(c.shape[0]), self.dim, kc, 0, ctypes.byref(n))
            need = max(need, n.value)
        new = lambda dt, *shape: torch.empty(*shape, dtype=dt, device=self.device)      # noqa: E731
        ws = new(torch.uint8, max(need, 8))
        idx, val = new(torch.int32, nq, k), new(torch.float32, nq, k)
        parts = None
        if len(self.chunks) > 1:
            parts = [(new(torch.int32, nq, kc), new(torch.float32, nq, kc)) for kc in ks]
        return ws, idx, val, parts

    def search(self, query8, k=20, copy=False):
        """query8 int8 device tensor [nq, dim] -> (idx int32 [nq, k], val float32 [nq, k]) device tensors, as
        `predict.search_reference(query8, gallery, inv_norm or None, k)` states them: the k best rows of every query, best first,
        and their scores (dot * inv_norm[row] for a cosine gallery: the cosine but for the query's own norm).  On the current
        stream, nothing synchronised.  The results are the gallery's own buffers for this (nq, k): copy=True (or clone) to keep
        them across calls.  1 <= k <= min(64, rows)."""
        assert isinstance(query8, torch.Tensor) and query8.dtype == torch.int8 and query8.is_contiguous() and query8.device == self.device
        assert query8.dim() == 2 and query8.shape[1] == self.dim, f"query8 must be [nq, {self.dim}]"
        k = int(k)
        if not 1 <= k <= min(MAX_K, self.rows):
            raise ValueError(f"k = {k} outside 1 .. min({MAX_K}, {self.rows})")
        nq = int(query8.shape[0])
        if nq == 0:
            return (torch.empty(0, k, dtype=torch.int32, device=self.device), torch.empty(0, k, dtype=torch.float32, device=self.device))
        self.h.set_stream(torch.cuda.current_stream(self.device).cuda_stream)
        ws, idx, val, parts = self._bufs.get((nq, k))
        for i, c in enumerate(self.chunks):
            oi, ov = (idx, val) if parts is None else parts[i]
            w = None if self.inv_norm is None else _P(self.inv_norm.data_ptr() + 4 * self.starts[i])
            self.h.call("ivit_search_topk", _ptr(query8), nq, _ptr(self._on_device(c)), int(c.shape[0]), self.dim, w, int(oi.shape[1]),
                        self.starts[i], 0, _ptr(ws), ws.numel(), _ptr(oi), _ptr(ov))
        if parts is not None:
            ci, cv = torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1)
            self.h.call("ivit_search_merge", _ptr(ci), _ptr(cv), nq, int(ci.shape[1]), k, _ptr(idx), _ptr(val))
        return (idx.clone(), val.clone()) if copy else (idx, val)

    def _inv_norms(self, feat8):
        """float32 [n] device tensor: ivit_gallery_inv_norms of any int8 rows on the device (the queries' weights for a cosine)"""
        out = torch.empty(int(feat8.shape[0]), dtype=torch.float32, device=self.device)
        self.h.call("ivit_gallery_inv_norms", _ptr(feat8), int(feat8.shape[0]), self.dim, _ptr(out))
        return out

    def _within(self, query8, qw, threshold, triangle, query_base, chunk_ids):
        """`within` over the chunks `chunk_ids` (ascending): count every chunk, ONE synchronisation for the totals, fill every chunk,
        then the rows of the chunks side by side in chunk order"""
        nq, dev = int(query8.shape[0]), self.device
        if nq == 0 or not chunk_ids:
            return (torch.zeros(nq + 1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                    torch.empty(0, dtype=torch.float32, device=dev))
        self.h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        n = ctypes.c_size_t()
        runs = []
        for i in chunk_ids:
            c = self.chunks[i]
            self.h.call("ivit_range_workspace_bytes", nq, int(c.shape[0]), self.dim, 0, ctypes.byref(n))
            ws = torch.empty(max(n.value, 8), dtype=torch.uint8, device=dev)
            row_ptr = torch.empty(nq + 1, dtype=torch.int64, device=dev)
            w = None if self.inv_norm is None else _P(self.inv_norm.data_ptr() + 4 * self.starts[i])
            args = (_ptr(query8), nq, None, int(c.shape[0]), self.dim, w, _ptr(qw), float(threshold), self.starts[i], int(query_base),
                    int(bool(triangle)), 0, _ptr(ws), ws.numel())
            self.h.call("ivit_range_count", *args[:2], _ptr(self._on_device(c)), *args[3:], _ptr(row_ptr))
            runs.append((c, args, row_ptr, ws))
        totals = torch.stack([r[2][nq] for r in runs]).cpu().tolist()          # the one synchronisation
        parts = []
        for (c, args, row_ptr, ws), total in zip(runs, totals):
            idx = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
            val = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
            self.h.call("ivit_range_fill", *args[:2], _ptr(self._on_device(c)), *args[3:], total, _ptr(idx), _ptr(val))
            parts.append((row_ptr, idx[:total], val[:total]))
        if len(parts) == 1:
            return parts[0]
        counts = torch.stack([p[0][1:] - p[0][:-1] for p in parts])             # [chunks, nq]
        row_ptr = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        row_ptr[1:] = counts.sum(0).cumsum(0)
        ahead = counts.cumsum(0) - counts                                        # a row's hits in the chunks before
        total = int(sum(totals))
        idx = torch.empty(total, dtype=torch.int32, device=dev)
        val = torch.empty(total, dtype=torch.float32, device=dev)
        rows_of = torch.arange(nq, device=dev)
        for j, ((rp, ci, cv), t) in enumerate(zip(parts, totals)):
            if t == 0:
                continue
            b = torch.repeat_interleave(rows_of, counts[j], output_size=t)
            dest = row_ptr[b] + ahead[j][b] + (torch.arange(t, device=dev) - rp[b])
            idx[dest] = ci
            val[dest] = cv
        return row_ptr, idx, val

    def within(self, query8, threshold, query_weight="auto", triangle=False, query_base=0):
        """query8 int8 device tensor [nq, dim] -> (row_ptr int64 [nq + 1], idx int32 [total], val float32 [total]) device tensors, as
        `predict.range_reference(query8, gallery, inv_norm or None, query_weight, threshold, 0, query_base, triangle)` states them:
        EVERY row of the gallery whose score against a query is >= threshold, by ascending row; row b is
        idx[row_ptr[b]:row_ptr[b + 1]].
        query_weight   "auto": for a cosine gallery the queries' inverse norms (ivit_gallery_inv_norms on query8), so that val is the
                       cosine; none for a dot-product gallery.  None, or a float32 device tensor [nq], otherwise.
        triangle       only the rows g with g > query_base + b: with the gallery's own rows as queries, every pair once.
        The order of work: ivit_range_count for every chunk (the chunk's first row as index_base), ONE SYNCHRONISATION to read the
        totals, the allocation of idx / val, ivit_range_fill for every chunk; a row's hits are the chunks' hits in chunk order (still
        ascending), laid side by side on the device.  The result does not depend on the chunking; the tensors are fresh."""
        assert isinstance(query8, torch.Tensor) and query8.dtype == torch.int8 and query8.is_contiguous() and query8.device == self.device
        assert query8.dim() == 2 and query8.shape[1] == self.dim, f"query8 must be [nq, {self.dim}]"
        if not np.isfinite(np.float32(threshold)):
            raise ValueError("threshold must be finite")
        if isinstance(query_weight, str):
            if query_weight != "auto":
                raise ValueError('query_weight: "auto", None or a float32 tensor [nq]')
            self.h.set_stream(torch.cuda.current_stream(self.device).cuda_stream)
            qw = self._inv_norms(query8) if self.cosine and query8.shape[0] else None
        else:
            qw = query_weight
            assert qw is None or (qw.dtype == torch.float32 and qw.is_contiguous() and qw.shape == (query8.shape[0],) and qw.device == self.device)
        return self._within(query8, qw, threshold, triangle, query_base, list(range(len(self.chunks))))


def _pairs_of(row_ptr, idx, first):
    """CSR rows -> int64 [total, 2]: (first + row, idx) for every entry, in the rows' order"""
    nq = row_ptr.shape[0] - 1
    counts = row_ptr[1:] - row_ptr[:-1]
    i = torch.repeat_interleave(torch.arange(nq, device=idx.device), counts, output_size=int(idx.shape[0])) + int(first)
    return torch.stack([i, idx.to(torch.int64)], 1)


def _join(queries, gallery, threshold, triangle):
    """every chunk of `queries` (a Gallery: its chunks, starts and device) against `gallery`, in order"""
    pairs, vals = [], []
    for a, c in enumerate(queries.chunks):
        q = c if c.is_cuda else c.to(gallery.device)                # a host chunk as queries: a copy of its own, not the staging buffer
        ids = [b for b in range(len(gallery.chunks)) if not triangle or gallery.starts[b + 1] - 1 > queries.starts[a]]
        row_ptr, idx, val = gallery._within(q, gallery._inv_norms(q) if gallery.cosine else None, threshold, triangle, queries.starts[a] if triangle else 0, ids)
        pairs.append(_pairs_of(row_ptr, idx, queries.starts[a]))
        vals.append(val)
    return torch.cat(pairs), torch.cat(vals)


def duplicates(feat8, threshold, cosine=True, chunk_rows=None):
    """feat8 int8 [N, dim] (or a list of chunks, as `Gallery` takes them) -> (pairs int64 [P, 2], val float32 [P]) device tensors: every
    pair i < j of rows whose cosine (cosine=False: whose exact integer dot product) is >= threshold, in lexicographic order, val as
    `predict.range_reference` states it with both rows' inverse norms.  The triangle self-join of include/ivit_range.h, chunk
    against chunk: chunk a's rows are the queries (query_base: its first row) of every chunk that reaches above a's first row; tiles
    at or below the diagonal are not loaded.  One synchronisation per query chunk.  The [N, N] matrix is never written."""
    gal = feat8 if isinstance(feat8, Gallery) else Gallery(feat8, cosine=cosine, chunk_rows=chunk_rows)
    gal.h.set_stream(torch.cuda.current_stream(gal.device).cuda_stream)
    return _join(gal, gal, threshold, True)


def cross_matches(feat8_a, feat8_b, threshold, cosine=True, chunk_rows=None):
    """the same without the triangle, between two sets: (pairs int64 [P, 2], val float32 [P]), every (i, j) with row i of feat8_a and row
    j of feat8_b at a cosine (dot product) >= threshold, in lexicographic order: the leakage check of a training set against a
    validation set.  feat8_b is the gallery (streamed), feat8_a the queries."""
    gal = feat8_b if isinstance(feat8_b, Gallery) else Gallery(feat8_b, cosine=cosine, chunk_rows=chunk_rows)
    qs = Gallery(feat8_a, cosine=False, chunk_rows=chunk_rows, device=gal.device)          # only its chunks and starts are used
    gal.h.set_stream(torch.cuda.current_stream(gal.device).cuda_stream)
    return _join(qs, gal, threshold, False)


def duplicate_groups(pairs, n):
    """pairs [P, 2] integers (rows of `duplicates`; any order, either orientation), n rows -> int64 [n] on the host: for every row the
    smallest index of its connected component (union-find by hooking every pair's larger label to the smaller and halving the paths,
    in numpy, until nothing changes).  `keep = group == np.arange(n)` is the deduplicated subset: one row per component."""
    pairs = (pairs.cpu().numpy() if isinstance(pairs, torch.Tensor) else np.asarray(pairs)).astype(np.int64).reshape(-1, 2)
    n = int(n)
    if pairs.size and (pairs.min() < 0 or pairs.max() >= n):
        raise ValueError(f"pairs name rows outside 0 .. {n - 1}")
    group = np.arange(n, dtype=np.int64)
    i, j = pairs[:, 0], pairs[:, 1]
    while True:
        low = np.minimum(group[i], group[j])
        new = group.copy()
        np.minimum.at(new, group[i], low)                           # hook the roots, and the rows themselves
        np.minimum.at(new, group[j], low)
        np.minimum.at(new, i, low)
        np.minimum.at(new, j, low)
        new = new[new]                                              # halve the paths
        if np.array_equal(new, group):
            return group
        group = new


def knn_classify(idx, val, labels, num_classes, T=0.07, query_inv_norm=None):
    """The weighted vote of the usual k-NN protocol for a frozen backbone, in torch float64 on the small [B, k] tensors: idx, val the
    results of a search, labels int64 [N] the gallery's labels, query_inv_norm float64 [B] (`query_inv_norms`) or None.
    cos[b, j] = float64(val[b, j]) * query_inv_norm[b] (val itself without it); neighbour j votes exp(cos[b, j] / T) for class
    labels[idx[b, j]], the votes of a class added in the order j = 0 .. k - 1.  Returns (order int64 [B, num_classes], vote float64
    [B, num_classes]): the classes by descending vote, equal votes by ascending class."""
    lab = labels[idx.to(torch.int64)]                                   # [B, k]
    cos = val.to(torch.float64)
    if query_inv_norm is not None:
        cos = cos * query_inv_norm.to(torch.float64).reshape(-1, 1)
    w = torch.exp(cos / float(T))
    vote = torch.zeros(idx.shape[0], int(num_classes), dtype=torch.float64, device=idx.device)
    for j in range(idx.shape[1]):                                       # one add per row and step: the order is j's, on any device
        vote.scatter_add_(1, lab[:, j:j + 1], w[:, j:j + 1])
    order = torch.sort(vote, dim=1, descending=True, stable=True)[1]
    return order, vote


def knn_reference(idx, val, labels, num_classes, T=0.07, query_inv_norm=None):
    """numpy statement of `knn_classify`: (order int64 [B, num_classes], vote float64 [B, num_classes])"""
    idx, labels = np.asarray(idx).astype(np.int64), np.asarray(labels).astype(np.int64)
    cos = np.asarray(val).astype(np.float64)
    if query_inv_norm is not None:
        cos = cos * np.asarray(query_inv_norm, dtype=np.float64).reshape(-1, 1)
    w = np.exp(cos / float(T))
    B, k = idx.shape
    vote = np.zeros((B, int(num_classes)), np.float64)
    for b in range(B):
        for j in range(k):
            vote[b, labels[idx[b, j]]] += w[b, j]
    cls = np.arange(int(num_classes))
    order = np.stack([np.lexsort((cls, -row)) for row in vote]).reshape(B, -1) if B else np.zeros((0, int(num_classes)), np.int64)
    return order.astype(np.int64), vote
