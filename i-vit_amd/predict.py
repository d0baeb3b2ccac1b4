"""Predictions: the output half of the reference's validate() (quant_train.py:314-351) on the device.

validate() multiplies the head's accumulators by the per-class head scale (quant_modules.py:96-97, returned unchanged by
vit_quant.py:278-282 / swin_quant.py:560-564), takes top-1 / top-5 against the labels and averages.  Here:

  * `topk_reference` is the numpy statement of the contract of `ivit_logits_topk` (include/ivit.h): values AND order;
  * the engines' `predict` / `capture_predict` (ivit_amd.native.NativeEngine: ivit_*_predict, ivit_*_predict_graph_create, the
    forward and the top-k launch as one C call, or one hipGraph) follow it;
  * `evaluate` is validate() minus the data loader and the loss: hit counts accumulate on the device, with device labels
    nothing inside the loop synchronises, and a multi-rank run ends with ONE all_reduce (no collective per step).
"""
import numpy as np
import torch

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
