"""Predictions: the output half of the reference's validate() (quant_train.py:314-351) on the device.

validate() multiplies the head's accumulators by the per-class head scale (quant_modules.py:96-97, returned unchanged by
vit_quant.py:278-282 / swin_quant.py:560-564), takes top-1 / top-5 against the labels and averages.  Here:

  * `topk_reference` is the numpy statement of the contract of `ivit_logits_topk` (include/ivit.h): values AND order;
  * `PredictMixin` gives ViTEngine and SwinEngine `predict` / `capture_predict` (ivit_*_predict, ivit_*_predict_graph_create:
    the forward and the top-k launch as one C call, or one hipGraph) and `head_scale_host`;
  * `evaluate` is validate() minus the data loader and the loss: hit counts accumulate on the device, with device labels
    nothing inside the loop synchronises, and a multi-rank run ends with ONE all_reduce (no collective per step).
"""
import ctypes

import numpy as np
import torch

_P = ctypes.c_void_p
MAX_K = 16          # TOPK_MAX_K of csrc/ivit_topk.h


def topk_reference(acc, scale, k):
    """acc int32 [B, ncls] (head accumulators), scale float32 [ncls] -> (idx int32 [B, k], val float32 [B, k]).

    v[b, c] = fl32(fl32(acc[b, c]) * scale[c]).  Descending by value, -0.0 and +0.0 equal, equal values by ascending class
    index: row b of idx is the first k entries of np.lexsort((arange(ncls), -(v[b] + 0.0))); val holds the bits of v
    (-0.0 stays -0.0).  Non-finite scale entries are outside the contract."""
    acc = np.asarray(acc)
    scale = np.asarray(scale, dtype=np.float32)
    assert acc.ndim == 2 and acc.dtype == np.int32 and scale.shape == (acc.shape[1],)
    ncls = acc.shape[1]
    if not 1 <= k <= min(MAX_K, ncls):
        raise ValueError(f"k = {k} outside 1 .. min({MAX_K}, {ncls})")
    v = acc.astype(np.float32) * scale[None, :]                       # int32 -> float32 is RNE; one float32 multiply
    cls = np.arange(ncls)
    idx = np.stack([np.lexsort((cls, -(row + np.float32(0.0))))[:k] for row in v]).astype(np.int32).reshape(-1, k)
    return idx, np.take_along_axis(v, idx.astype(np.int64), axis=1)


class PredictMixin:
    """predict / capture_predict / head_scale_host of an engine that has h, model, device, cfg, table, blob, ptr(),
    _native_buffers() with its cache _native_ws, and MAX_SLICES, and names its C entries in _PREDICT / _PREDICT_GRAPH."""

    def head_scale_host(self):
        """host float32 copy [num_classes] of the head's scale (the reference's head.bias_scaling_factor), read from the device
        once; every call returns a fresh array, the caller's to change.  The one spelling both engines share:
        ViTEngine.head_scale() and SwinEngine.head_scale stay as they were."""
        if getattr(self, "_head_scale_host", None) is None:
            o, _, shp = self.table["head.scale"]
            self._head_scale_host = self.blob[o:o + 4 * int(np.prod(shp))].cpu().numpy().view(np.float32).copy()
        return self._head_scale_host.copy()

    def _predict_buffers(self, B, nslices, k):
        """(workspace, logits, idx, val) of one (batch, slices, k): idx / val live beside the logits buffer and follow its rule —
        the engine's own, overwritten by the next call of the same shape, pinned while a captured graph refers to them"""
        ws, logits = self._native_buffers(B, nslices)
        outs = self.__dict__.setdefault("_predict_out", {})
        key = (B, nslices, k)
        hit = outs.get(key)
        if hit is None or hit[0] is not logits:          # first use, or the logits buffer of this shape was evicted and rebuilt
            for old in [q for q, v in outs.items() if not v[3] and (q[0], q[1]) not in self._native_ws]:
                del outs[old]
            hit = outs[key] = [logits, torch.empty(B, k, dtype=torch.int32, device=self.device),
                               torch.empty(B, k, dtype=torch.float32, device=self.device), False]
        return ws, logits, hit[1], hit[2]

    def _predict_args(self, images, nslices, k):
        assert images.dtype == torch.int8 and images.is_contiguous() and images.device == self.device
        B = images.shape[0]
        nslices = max(1, min(int(nslices), B, self.MAX_SLICES))
        ws, logits, idx, val = self._predict_buffers(B, nslices, int(k))
        args = (self.model, _P(images.data_ptr()), B, nslices, _P(ws.data_ptr()), ws.numel(), _P(logits.data_ptr()),
                self.ptr("head.scale"), int(k), _P(idx.data_ptr()), _P(val.data_ptr()))
        return args, (B, nslices, int(k)), (ws, logits, idx, val)

    def predict(self, images, k=5, nslices=1, copy=False):
        """images int8 [B, C, H, W] -> (idx int32 [B, k], val float32 [B, k]) device tensors: the k best classes of every image in
        the order of `topk_reference`, and their dequantised head outputs.  One native call (the forward, then the top-k launch
        behind the slices' join); the head scale is read where it lies in the constants blob.  The int32 logits of the same call
        are in `last_logits`.  Like forward(), the results are the engine's own buffers for this (batch, nslices, k): copy=True
        (or clone) to keep them across calls.  1 <= k <= min(16, num_classes)."""
        self.h.set_stream(torch.cuda.current_stream(self.device).cuda_stream)
        args, _, (_, logits, idx, val) = self._predict_args(images, nslices, k)
        self.h._check(getattr(self.h.lib, self._PREDICT)(*args), self._PREDICT)
        self.last_logits = logits
        return (idx.clone(), val.clone()) if copy else (idx, val)

    def capture_predict(self, images, k=5, nstreams=1):
        """hipGraph of one predict on fixed buffers; returns a callable that replays it and returns (idx, val)."""
        args, key, keep = self._predict_args(images, nstreams, k)
        if not hasattr(self, "_gstream"):
            self._gstream = torch.cuda.Stream(self.device)
        torch.cuda.synchronize(self.device)
        self.h.set_stream(self._gstream.cuda_stream)
        g = _P()
        self.h._check(getattr(self.h.lib, self._PREDICT_GRAPH)(*args, ctypes.byref(g)), self._PREDICT_GRAPH)
        # the graph has its buffers baked in: they live as long as the replay closure, and their cache entries are pinned
        self._graphs = getattr(self, "_graphs", []) + [(g,) + keep + (images,)]
        self._graph_keys = getattr(self, "_graph_keys", set()) | {key[:2]}
        self._predict_out[key][3] = True
        lib, gs, dev, idx, val = self.h.lib, self._gstream, self.device, keep[2], keep[3]

        def replay(_keep=keep + (images,)):
            cur = torch.cuda.current_stream(dev)
            gs.wait_stream(cur)
            self.h.set_stream(gs.cuda_stream)
            self.h._check(lib.ivit_graph_launch(g), "ivit_graph_launch")
            cur.wait_stream(gs)
            return idx, val
        return replay


def evaluate(engine, batches, topk=(1, 5), transform=None, rank=0, world=1):
    """validate() of the reference (quant_train.py:314-351) without its data loader and loss.

    `batches` yields (images, labels) — with world > 1, THIS rank's share of them (ivit_amd.dist.shard_range); `transform`
    turns what it yields into the engine's int8 input (e.g. lambda u8: eval_transform(u8, s_in)); labels are class indices [B].
    Runs engine.predict(k = max(topk), clamped to num_classes: a 10-class model has no top-16) and counts, for every j of
    `topk`, the images whose label is among the first j indices.  The hit counts accumulate in ONE int64 tensor on the
    predictions' device; the image count is a host integer that joins them after the loop.  With labels already on that
    device nothing inside the loop synchronises or copies between host and device: the host runs ahead of the GPU.  Host
    labels are uploaded batch by batch (non_blocking, but from pageable memory the runtime may still hold the host until the
    stream reaches the copy) — upload a rank's labels once instead, as dist.evaluate_sharded and tools/evaluate.py do.
    world > 1 ends with one all_reduce(SUM).
    Returns {"n": images, "correct": {j: count}, "acc": {j: 100 * count / n}} (the reference's Prec@j)."""
    topk = tuple(int(j) for j in topk)
    if not topk or min(topk) < 1:
        raise ValueError("topk must name ranks >= 1")
    k = min(max(topk), int(engine.cfg.num_classes))
    n, hits = 0, None                                                   # hits[t]: images whose label is among the first topk[t]
    for images, labels in batches:
        if transform is not None:
            images = transform(images)
        idx = torch.as_tensor(engine.predict(images, k=k)[0])
        labels = torch.as_tensor(labels).to(device=idx.device, dtype=torch.int64, non_blocking=True).reshape(-1, 1)
        within = (idx.to(torch.int64) == labels).cumsum(1) > 0         # [B, k]: label among the first j + 1 indices
        step = torch.stack([within[:, min(j, k) - 1].sum() for j in topk])
        hits = step if hits is None else hits + step
        n += idx.shape[0]
    if hits is None:                                                    # an empty share still joins the reduction
        hits = torch.zeros(len(topk), dtype=torch.int64, device=getattr(engine, "device", "cpu"))
    counts = torch.cat([torch.tensor([n], dtype=torch.int64, device=hits.device), hits])     # [n, hits of topk[0], ...]
    if world > 1:
        import torch.distributed as dist
        if not dist.is_initialized():
            raise RuntimeError(f"evaluate(rank={rank}, world={world}) needs an initialised process group")
        if dist.get_backend() == "gloo":                               # gloo reduces host tensors
            counts = counts.cpu()
        dist.all_reduce(counts, op=dist.ReduceOp.SUM)
    c = [int(v) for v in counts.cpu().tolist()]
    n = c[0]
    correct = {j: c[1 + t] for t, j in enumerate(topk)}
    return {"n": n, "correct": correct, "acc": {j: (100.0 * v / n if n else float("nan")) for j, v in correct.items()}}
