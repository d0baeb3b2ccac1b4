"""Predictions: the output half of the reference's validate() (quant_train.py:314-351) on the device.

validate() multiplies the head's accumulators by the per-class head scale (quant_modules.py:96-97, returned unchanged by
vit_quant.py:278-282 / swin_quant.py:560-564), takes the cross-entropy and top-1 / top-5 against the labels and averages.  Here:

  * `topk_reference` is the numpy statement of the contract of `ivit_logits_topk` (include/ivit.h): values AND order;
  * `score_reference` is the numpy statement of the contract of `ivit_logits_score` (include/ivit_eval.h): per image, the rank of
    the label in that order and its negative log-likelihood in fp64;
  * the engines' `predict` / `capture_predict` and `score` / `capture_score` (ivit_amd.native.NativeEngine: ivit_*_predict,
    ivit_*_score and their *_graph_create forms, the forward and the launch behind it as one C call, or one hipGraph) follow them;
  * `evaluate` is validate() minus the data loader: hit counts — and with loss=True the sum of the losses — accumulate on the
    device, with device labels nothing inside the loop synchronises, and a multi-rank run ends with ONE all_reduce (DESIGN.md §6:
    no collective per step);
  * `features_reference` is the numpy statement of the contract of `ivit_features_f32` (include/ivit_features.h): the fp32 form of
    the int8 features the reference's forward_features returns (vit_quant.py:254-276, swin_quant.py:540-556), and `embed` is
    evaluate's loop for them (the engines' `features`).
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


def score_reference(acc, scale, labels):
    """acc int32 [B, ncls], scale float32 [ncls], labels integers [B] -> (rank int32 [B], nll float64 [B]).

    v as in `topk_reference`.  rank[b] is the number of classes strictly before labels[b] in the order of `topk_reference`
    (descending value, -0.0 and +0.0 equal, ties by ascending class index), so topk_reference(acc, scale, k)[0][b, rank[b]] ==
    labels[b] whenever rank[b] < k.  With d = float64(v[b]) and m = max(d): nll[b] = log(sum(exp(d - m))) - (d[labels[b]] - m),
    everything in float64 — F.cross_entropy(v.double(), labels, reduction="none").  A label outside [0, ncls) gives
    rank = INT32_MAX and nll = NaN.  Non-finite scale entries are outside the contract."""
    acc = np.asarray(acc)
    scale = np.asarray(scale, dtype=np.float32)
    labels = np.asarray(labels).astype(np.int64).reshape(-1)
    assert acc.ndim == 2 and acc.dtype == np.int32 and scale.shape == (acc.shape[1],) and labels.shape == (acc.shape[0],)
    B, ncls = acc.shape
    assert ncls >= 1
    v = acc.astype(np.float32) * scale[None, :]                       # int32 -> float32 is RNE; one float32 multiply
    valid = (labels >= 0) & (labels < ncls)
    lc = np.where(valid, labels, 0)
    rows, cls = np.arange(B), np.arange(ncls)[None, :]
    key = v + np.float32(0.0)                                         # -0.0 -> +0.0: the two compare equal anyway, as the order says
    lv = key[rows, lc][:, None]
    before = ((key > lv) | ((key == lv) & (cls < lc[:, None]))).sum(axis=1)
    d = v.astype(np.float64)
    m = d.max(axis=1, keepdims=True)
    nll = np.log(np.exp(d - m).sum(axis=1)) - (d[rows, lc] - m[:, 0])
    return (np.where(valid, before, np.iinfo(np.int32).max).astype(np.int32), np.where(valid, nll, np.nan).astype(np.float64))


def features_reference(feat8, scale, mode=0):
    """feat8 int8 [B, dim], scale a float32 value -> float32 [B, dim], every bit.

    mode 0 (IVIT_FEATURES_DEQUANT): fl32(fl32(q) * scale), one conversion and one float32 multiply: the fp32 tensor QuantAct
    returns in the reference (quant_modules.py:197-206).  mode 1 (IVIT_FEATURES_UNIT): rows of unit Euclidean length; the scale
    cancels and is not read: ss = sum of q^2 as an exact integer, fl32(float64(q) / sqrt(float64(ss))) with the correctly rounded
    float64 root and division numpy has; a row of zeros gives zeros.  The scale must be finite and positive in both modes."""
    q = np.asarray(feat8)
    scale = np.float32(scale)
    assert q.ndim == 2 and q.dtype == np.int8
    if mode not in (0, 1):
        raise ValueError(f"mode = {mode}: 0 (dequantised) or 1 (unit length)")
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError(f"scale = {scale}: finite and positive")
    if mode == 0:
        return q.astype(np.float32) * scale
    ss = (q.astype(np.int64) ** 2).sum(axis=1)
    root = np.sqrt(np.where(ss > 0, ss, 1).astype(np.float64))        # a row of zeros: 0 / 1
    return (q.astype(np.float64) / root[:, None]).astype(np.float32)


def embed(engine, batches, transform=None, normalize=True):
    """evaluate's loop for features: `batches` yields images, or (images, anything) pairs as evaluate takes them; `transform`
    turns what it yields into the engine's int8 input.  Every batch is one engine.features(images, normalize=normalize) — no
    head GEMM — and its fp32 rows are kept (a copy: the engine reuses its buffers), in order.  Nothing inside the loop
    synchronises.  Returns ONE float32 tensor [N, num_features] on the engine's device ([0, num_features] without batches):
    unit-length rows by default (dot products are cosines), feat8 * scale with normalize=False."""
    rows = []
    for images in batches:
        if isinstance(images, (tuple, list)):
            images = images[0]
        if transform is not None:
            images = transform(images)
        rows.append(torch.as_tensor(engine.features(images, normalize=normalize)[1]).clone())
    if not rows:
        return torch.zeros(0, int(engine.num_features), dtype=torch.float32, device=getattr(engine, "device", "cpu"))
    return torch.cat(rows)


def evaluate(engine, batches, topk=(1, 5), transform=None, rank=0, world=1, loss=False):
    """validate() of the reference (quant_train.py:314-351) without its data loader — and, unless loss=True, without its loss.

    `batches` yields (images, labels) — with world > 1, THIS rank's share of them (ivit_amd.dist.shard_range); `transform`
    turns what it yields into the engine's int8 input (e.g. lambda u8: eval_transform(u8, s_in)); labels are class indices [B].
    Runs engine.predict(k = max(topk), clamped to num_classes: a 10-class model has no top-16) and counts, for every j of
    `topk`, the images whose label is among the first j indices.  The hit counts accumulate in ONE int64 tensor on the
    predictions' device; the image count is a host integer that joins them after the loop.  With labels already on that
    device nothing inside the loop synchronises or copies between host and device: the host runs ahead of the GPU.  Host
    labels are uploaded batch by batch (non_blocking, but from pageable memory the runtime may still hold the host until the
    stream reaches the copy) — upload a rank's labels once instead, as dist.evaluate_sharded and tools/evaluate.py do.
    world > 1 ends with one all_reduce(SUM).
    Returns {"n": images, "correct": {j: count}, "acc": {j: 100 * count / n}} (the reference's Prec@j).

    loss=True is the whole of validate(): it runs engine.score instead (rank and negative log-likelihood of every label, one
    launch behind the forward), counts the images with rank < j — any j, no top-k and no clamp — and adds the losses into a
    float64 scalar on the device.  The loop synchronises as little as the other; the counts and the sum travel as ONE float64
    tensor [n, hits..., loss_sum] (integers are exact there up to 2^53) through the one all_reduce.  Returns the same dict
    plus "loss": loss_sum / n, the reference's `Loss` (NaN if a label lies outside the classes)."""
    topk = tuple(int(j) for j in topk)
    if not topk or min(topk) < 1:
        raise ValueError("topk must name ranks >= 1")
    if loss:
        return _evaluate_with_loss(engine, batches, topk, transform, rank, world)
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


def _evaluate_with_loss(engine, batches, topk, transform, rank, world):
    """evaluate(loss=True): see there"""
    n, sums = 0, None                                                   # sums: [hits of topk[0], ..., loss_sum] in float64
    for images, labels in batches:
        if transform is not None:
            images = transform(images)
        device = getattr(engine, "device", "cpu")
        labels = torch.as_tensor(labels).to(device=device, dtype=torch.int64, non_blocking=True).reshape(-1)
        rk, nll = (torch.as_tensor(t) for t in engine.score(images, labels))
        step = torch.stack([(rk < j).sum().to(torch.float64) for j in topk] + [nll.to(torch.float64).sum()])
        sums = step if sums is None else sums + step
        n += rk.shape[0]
    if sums is None:                                                    # an empty share still joins the reduction
        sums = torch.zeros(len(topk) + 1, dtype=torch.float64, device=getattr(engine, "device", "cpu"))
    totals = torch.cat([torch.tensor([n], dtype=torch.float64, device=sums.device), sums])       # [n, hits ..., loss_sum]
    if world > 1:
        import torch.distributed as dist
        if not dist.is_initialized():
            raise RuntimeError(f"evaluate(rank={rank}, world={world}) needs an initialised process group")
        if dist.get_backend() == "gloo":                               # gloo reduces host tensors
            totals = totals.cpu()
        dist.all_reduce(totals, op=dist.ReduceOp.SUM)
    c = totals.cpu().tolist()
    n = int(c[0])
    correct = {j: int(c[1 + t]) for t, j in enumerate(topk)}
    return {"n": n, "correct": correct, "acc": {j: (100.0 * v / n if n else float("nan")) for j, v in correct.items()},
            "loss": c[-1] / n if n else float("nan")}
