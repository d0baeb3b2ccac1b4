"""Gallery search over the engines' int8 features (include/ivit_search.h): `Gallery` holds the rows (and, for cosine, their inverse
norms) and finds every query's k nearest through `ivit_search_topk` — the gallery streamed once, the scores never written — chunk by
chunk with `ivit_search_merge` behind when it was given in pieces; `knn_classify` is the weighted vote of the usual k-NN protocol
for a frozen backbone on the small [B, k] results, `knn_reference` its numpy statement.  The numpy statements of the search itself
are `predict.search_reference` and `predict.inv_norms_reference`.  torch is used for device memory and streams, and for the vote."""
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
