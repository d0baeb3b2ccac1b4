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
  * `view_sum_reference` is the numpy statement of the contract of `ivit_logits_view_sum` (include/ivit_views.h): the integer sum of
    the logits of the views of one image (ivit_amd/views.py); the engines' `predict_views` / `score_views` and
    `evaluate(..., views=V)` are `predict` / `score` / `evaluate` on the mean logits of V views per image;
  * `features_reference` is the numpy statement of the contract of `ivit_features_f32` (include/ivit_features.h): the fp32 form of
    the int8 features the reference's forward_features returns (vit_quant.py:254-276, swin_quant.py:540-556), and `embed` is
    evaluate's loop for them (the engines' `features`);
  * `attention_reference` is the numpy statement of the contract of `ivit_attention_cls_probs` (include/ivit_attnmap.h): row 0 of
    IntSoftmax's output (vit_quant.py:70-76, quant_modules.py:469-497) from a block's q and k, and `attention_map_reference` that of
    `ivit_attention_map_f32`, the fp32 map over the patches (ViTEngine's `attention`);
  * `class_map_reference` is the numpy statement of the contract of `ivit_class_map` (include/ivit_classmap.h): a Swin's
    class-activation maps, the head's weight rows against every final-stage token, in exact integers (SwinEngine's `class_map`);
  * `hidden_reference` is the numpy statement of the contract of `ivit_hidden_f32` (include/ivit_hidden.h): the fp32 form of a
    block's or a stage's 16-bit output, the integers times the site's scale (the engines' `hidden_states`);
  * `search_reference` and `inv_norms_reference` are the numpy statements of the contracts of `ivit_search_topk` and
    `ivit_gallery_inv_norms` (include/ivit_search.h): the k nearest rows of an int8 gallery by exact dot product or by cosine
    (`ivit_amd.search.Gallery`, the engines' `retrieve`); `embed8` is `embed`'s loop keeping the integers, `knn_evaluate` is
    `evaluate`'s with the weighted k-NN vote (`ivit_amd.search.knn_classify`) in place of the head.
"""
import numpy as np
import torch

# the numpy statements of include/ivit_jpeg.h (both halves of the decoder) live in ivit_amd/jpeg.py, as views_reference does in
# views.py; they are named here beside the others
from .jpeg import jpeg_coefficients_reference, jpeg_reference  # noqa: F401

MAX_K = 16         # TOPK_MAX_K of csrc/ivit_topk.h


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


MAX_VIEWS = 64      # VIEW_SUM_MAX_VIEWS of csrc/ivit_views.h


def view_sum_reference(acc, views):
    """acc int32 [G * views, ncls], the views of an image in consecutive rows -> int32 [G, ncls]: the contract of
    `ivit_logits_view_sum` (include/ivit_views.h).  Row g is the sum of rows g * views .. g * views + views - 1 in int64, saturated to
    int32.  The views share the head's per-class scale, so `topk_reference` / `score_reference` of the sum with
    `view_scale_reference(scale, views)` are the values, the order and the loss of the MEAN logits."""
    acc = np.asarray(acc)
    assert acc.ndim == 2 and acc.dtype == np.int32
    if not 1 <= views <= MAX_VIEWS:
        raise ValueError(f"views = {views} outside 1 .. {MAX_VIEWS}")
    if acc.shape[0] % views:
        raise ValueError(f"{acc.shape[0]} rows are no multiple of {views} views")
    s = acc.reshape(acc.shape[0] // views, views, acc.shape[1]).astype(np.int64).sum(axis=1)
    return np.clip(s, np.iinfo(np.int32).min, np.iinfo(np.int32).max).astype(np.int32)


def view_scale_reference(scale, views):
    """the scale vector that goes with a sum over `views` views: fl32(scale / fl32(views)), one float32 division per class"""
    return (np.asarray(scale, dtype=np.float32) / np.float32(views)).astype(np.float32)


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


def _dyadic_mr(dy):
    """(m, r) as float64 from a pair, a [1, 2] array or anything with .m and .r (a Dyadic, or a one-element array of them)"""
    if hasattr(dy, "m"):
        return np.float64(dy.m), np.float64(dy.r)
    if not isinstance(dy, np.ndarray) and hasattr(dy, "__len__") and len(dy) == 1 and hasattr(dy[0], "m"):
        return np.float64(dy[0].m), np.float64(dy[0].r)
    m, r = np.asarray(dy, dtype=np.float64).reshape(2)
    return m, r


def _torch_order_sum(e):
    """float32 [R, n] -> float32 [R]: the sum over the last axis in the order torch's CPU kernel adds a contiguous float32 row
    (torch_order_sum32 of csrc/ivit_device.h is the same statement): 32 accumulators, element 32 i + a into
    accumulator a, closed into a second level every 16 steps, a third every 256; whole 8-vectors left over into accumulators 0..7;
    p[l] = ((a[l] + a[8 + l]) + a[16 + l]) + a[24 + l]; the scalar tail summed first, then p[0] .. p[7] onto it.  Every addition
    rounds to float32."""
    e = np.ascontiguousarray(e, dtype=np.float32)
    R, n = e.shape
    nvec, size = n >> 3, n >> 5
    a0, a1, a2, a3 = (np.zeros((R, 32), np.float32) for _ in range(4))
    i = 0
    while i + 16 <= size:
        for _ in range(16):
            a0 = a0 + e[:, 32 * i:32 * i + 32]
            i += 1
        a1, a0 = a1 + a0, np.zeros_like(a0)
        if i & 0xF0:
            continue
        a2, a1 = a2 + a1, np.zeros_like(a1)
        if i & 0xF00:
            continue
        a3, a2 = a3 + a2, np.zeros_like(a2)
    while i < size:
        a0 = a0 + e[:, 32 * i:32 * i + 32]
        i += 1
    a0 = ((a0 + a1) + a2) + a3
    for v in range(size * 4, nvec):
        a0[:, :8] = a0[:, :8] + e[:, 8 * v:8 * v + 8]
    p = ((a0[:, 0:8] + a0[:, 8:16]) + a0[:, 16:24]) + a0[:, 24:32]
    fin = np.zeros(R, np.float32)
    for k in range(nvec * 8, n):
        fin = fin + e[:, k]
    if nvec:
        for l in range(8):
            fin = fin + p[:, l]
    assert fin.dtype == np.float32
    return fin


def attention_reference(q, k, dy_qk, s_softmax):
    """q, k int8 [BH, T, dh] (a block's query and key, one [T, dh] per image and head), dy_qk the multiplier (m, r) of qact_attn1,
    s_softmax its scale -> uint16 [BH, T]: the class token's attention probabilities, row 0 of IntSoftmax's output, scale 2^-15.

    acc[j] = q[0] . k[j] as an exact integer; sc8 = clip(rint((float64(acc) * m) * r), -128, 127) (quant_utils.py:229-251).  Then
    IntSoftmax.forward in float32, one rounding per operation (quant_modules.py:469-497): x = fl(fl(sc8 * s) / s) minus its row
    maximum; t = max(x + floor(x / 2) - floor(x / 16), 15 x0) with x0 = floor(-1 / s); qq = floor(t / x0); e = max(floor((fl(t - x0 qq) / 2
    - x0) * 2^(15 - qq)), 0); S = min(sum e, 2^31) in torch's order; F = floor(fl(1 / S) * 2^31); p = floor(fl(e * F) / 2^16).  Of q only
    row 0 is read."""
    f32 = np.float32
    q, k = np.asarray(q), np.asarray(k)
    assert q.dtype == np.int8 and k.dtype == np.int8 and q.ndim == 3 and q.shape == k.shape
    s = f32(s_softmax)
    if not (np.isfinite(s) and s > 0):
        raise ValueError(f"s_softmax = {s}: finite and positive")
    m, r = _dyadic_mr(dy_qk)
    acc = np.einsum("bd,bjd->bj", q[:, 0].astype(np.int64), k.astype(np.int64))
    sc8 = np.clip(np.rint((acc.astype(np.float64) * m) * r), -128, 127).astype(f32)
    xt = (sc8 * s) / s
    x = xt - xt.max(axis=1, keepdims=True)
    x0 = np.floor(f32(-1.0) / s)
    t = x + np.floor(x * f32(0.5))
    t = np.maximum(t - np.floor(x * f32(0.0625)), f32(15.0) * x0)
    qq = np.floor(t / x0)
    e = (t - x0 * qq) * f32(0.5) - x0
    e = np.maximum(np.floor(np.ldexp(e, (15 - qq).astype(np.int32))), f32(0.0))
    assert xt.dtype == t.dtype == e.dtype == f32
    S = np.minimum(_torch_order_sum(e), f32(2147483648.0))
    F = np.floor((f32(1.0) / S) * f32(2147483648.0))
    p = np.floor((e * F[:, None]) * f32(2.0 ** -16))
    assert p.dtype == f32
    return p.astype(np.uint16)


def attention_map_reference(attn16, heads=False):
    """attn16 uint16 [..., H, T] -> float32, the patch columns 1 .. T - 1 only, every bit.

    heads=True (IVIT_ATTNMAP_HEADS): [..., H, T - 1], p * 2^-15, exact: the float32 tensor IntSoftmax returns in the reference.
    heads=False (IVIT_ATTNMAP_MEAN): [..., T - 1], the mean over the heads: S = sum_h p as an exact integer, float64(S) /
    float64(H * 32768) rounded ONCE to float32 (S and H * 32768 are below 2^24: this is the correctly rounded float32 quotient)."""
    p = np.asarray(attn16)
    assert p.dtype == np.uint16 and p.ndim >= 2
    H = p.shape[-2]
    if not 1 <= H <= 511:
        raise ValueError(f"{H} heads: 1 .. 511 (the sum must stay below 2^24)")
    p = p[..., 1:]
    if heads:
        return p.astype(np.float32) * np.float32(2.0 ** -15)
    S = p.astype(np.int64).sum(axis=-2)
    return (S.astype(np.float64) / np.float64(H * 32768)).astype(np.float32)


def class_map_reference(tok8, head_w, idx, class_scale=None):
    """tok8 int8 [B, L, C] (a Swin's final-stage tokens behind norm -> qact2, swin_quant.py:551-552), head_w int8 [num_classes, C] (the
    head's weight_integer, quant_modules.py:67-83), idx int32 [B, k] -> (cam32 int32 [B, k, L], map32 float32 [B, k, L] or None).

    cam32[b, j, t] = sum_c int(head_w[idx[b, j], c]) * int(tok8[b, t, c]), an exact integer: |cam32| <= 128 * 127 * C < 2^24 for
    C <= 1024, the limit of the entry.  With class_scale float32 [num_classes] = fl32(s_tok * fc_scaling_factor) (quant_modules.py:96-97
    with qact2's scale in place of qact3's): map32 = fl32(fl32(cam32) * class_scale[idx]), an exact conversion and ONE float32
    multiply, the contract of `topk_reference`'s v.  An index outside [0, num_classes) gives a cam32 row of zeros and a map32 row of
    NaN (`score_reference`'s convention for such a label); duplicate indices in a row are allowed.

    The exact identity behind the maps: sum_t cam32[b, j, t] == head_w[c] . sum_t tok8[b, t, :].  The pool's requantisation of that
    token sum (swin_quant.py:553-555) is what the head reads, so the sum of a map explains logits - bias up to that single
    requantisation."""
    tok8, head_w, idx = np.asarray(tok8), np.asarray(head_w), np.asarray(idx)
    assert tok8.dtype == np.int8 and tok8.ndim == 3 and head_w.dtype == np.int8 and head_w.ndim == 2 and head_w.shape[1] == tok8.shape[2]
    assert idx.dtype == np.int32 and idx.ndim == 2 and idx.shape[0] == tok8.shape[0]
    ncls, C = head_w.shape
    if C % 16 or C > 1024:
        raise ValueError(f"C = {C}: a multiple of 16, at most 1024 (the sums must stay below 2^24)")
    valid = (idx >= 0) & (idx < ncls)
    rows = head_w[np.where(valid, idx, 0)].astype(np.int64)                  # [B, k, C]
    cam = np.einsum("bjc,btc->bjt", rows, tok8.astype(np.int64))
    cam32 = np.where(valid[:, :, None], cam, 0).astype(np.int32)
    if class_scale is None:
        return cam32, None
    class_scale = np.asarray(class_scale)
    assert class_scale.dtype == np.float32 and class_scale.shape == (ncls,)
    map32 = cam32.astype(np.float32) * class_scale[np.where(valid, idx, 0)][:, :, None]
    assert map32.dtype == np.float32
    return cam32, np.where(valid[:, :, None], map32, np.float32(np.nan)).astype(np.float32)


def hidden_reference(q16, scale, layout="tokens", t0=0):
    """q16 int16 [B, T, C] (the integers of a block's closing QuantAct, qact4: vit_quant.py:141-143, SwinTransformerBlock.forward),
    scale the site's per-tensor scale -> float32 [B, T - t0, C] (layout "tokens") or [B, C, T - t0] (layout "grid", channel-major:
    the caller views the last axis as gh x gw).

    out = fl32(fl32(q) * scale) for the rows t0 .. T - 1 of every image: the conversion of an int16 is exact, then ONE float32
    multiply — the tensor QuantAct.forward returns in the reference (x = q * s, quant_modules.py:204-206), bit for bit.  t0 = 1
    drops a ViT's class row.  The grid form is the transpose of the tokens form, nothing else.  scale must be finite and positive,
    C a multiple of 8 (the limits of the entry)."""
    q16 = np.asarray(q16)
    assert q16.dtype == np.int16 and q16.ndim == 3
    B, T, C = q16.shape
    scale = np.float32(scale)
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError(f"scale = {scale!r}: finite and positive")
    if C % 8:
        raise ValueError(f"C = {C}: a multiple of 8")
    if not 0 <= t0 < T:
        raise ValueError(f"t0 = {t0}: in [0, {T})")
    if layout not in ("tokens", "grid"):
        raise ValueError(f"layout = {layout!r}: 'tokens' or 'grid'")
    out = q16[:, t0:, :].astype(np.float32) * scale
    assert out.dtype == np.float32
    return np.ascontiguousarray(out if layout == "tokens" else out.transpose(0, 2, 1))


SEARCH_MAX_K = 64   # SEARCH_MAX_K of csrc/ivit_search.h


def inv_norms_reference(gallery8):
    """gallery8 int8 [rows, dim] -> float32 [rows], every bit: ss = sum of q^2 as an exact integer, fl32(1.0 / sqrt(float64(ss))) with
    the correctly rounded float64 root and division numpy has, rounded to float32 once; a row of zeros gives +0.0 (the idiom of
    `features_reference`, mode 1).  As the `weight` of `search_reference` it makes the order of a query's neighbours the cosine
    order."""
    g = np.asarray(gallery8)
    assert g.ndim == 2 and g.dtype == np.int8
    ss = (g.astype(np.int64) ** 2).sum(axis=1)
    inv = np.float64(1.0) / np.sqrt(np.where(ss > 0, ss, 1).astype(np.float64))
    return np.where(ss > 0, inv, 0.0).astype(np.float32)


def search_reference(query8, gallery8, weight, k, index_base=0):
    """query8 int8 [nq, dim], gallery8 int8 [rows, dim], weight float32 [rows] or None -> (idx int32 [nq, k], val float32 [nq, k]).

    dot[b, g] = query8[b] . gallery8[g] as an exact integer (|dot| <= 2^24 for dim <= 1024: its float32 form is exact);
    v[b, g] = fl32(fl32(dot) * weight[g]), or fl32(dot) without a weight.  The order is `topk_reference`'s: descending by value,
    -0.0 and +0.0 equal, equal values by ascending gallery index: row b of idx is index_base + the first k entries of
    np.lexsort((arange(rows), -(v[b] + 0.0))); val holds the bits of v.  1 <= k <= min(64, rows); index_base >= 0 and
    index_base + rows <= 2^31 - 1.  It is `topk_reference` on the dot products wherever both apply (k <= 16)."""
    q, g = np.asarray(query8), np.asarray(gallery8)
    assert q.ndim == 2 and g.ndim == 2 and q.dtype == np.int8 and g.dtype == np.int8 and q.shape[1] == g.shape[1]
    rows = g.shape[0]
    if not 1 <= k <= min(SEARCH_MAX_K, rows):
        raise ValueError(f"k = {k} outside 1 .. min({SEARCH_MAX_K}, {rows})")
    if index_base < 0 or index_base + rows > 2 ** 31 - 1:
        raise ValueError(f"index_base = {index_base}: >= 0 and index_base + rows <= 2^31 - 1")
    dot = q.astype(np.int32) @ g.astype(np.int32).T
    v = dot.astype(np.float32)
    if weight is not None:
        weight = np.asarray(weight, dtype=np.float32)
        assert weight.shape == (rows,)
        v = v * weight[None, :]                                       # one float32 multiply
    assert v.dtype == np.float32
    cols = np.arange(rows)
    idx = np.stack([np.lexsort((cols, -(row + np.float32(0.0))))[:k] for row in v]).reshape(-1, k) if len(v) else np.zeros((0, k), np.int64)
    val = np.take_along_axis(v, idx.astype(np.int64), axis=1)
    return (idx + index_base).astype(np.int32), val


def range_reference(query8, gallery8, weight, qweight, threshold, index_base=0, query_base=0, triangle=False):
    """query8 int8 [nq, dim], gallery8 int8 [rows, dim], weight float32 [rows] or None, qweight float32 [nq] or None -> (row_ptr int64
    [nq + 1], idx int32 [total], val float32 [total]): the numpy statement of include/ivit_range.h.

    dot[b, g] = query8[b] . gallery8[g] as an exact integer; v[b, g] = fl32(fl32(fl32(dot) * weight[g]) * qweight[b]), two float32
    multiplies in this order, a None weight / qweight that multiply left out.  (b, g) is a hit if v[b, g] >= threshold (the IEEE
    comparison: -0.0 >= +0.0 holds) and, with triangle, index_base + g > query_base + b.  Row b of the result holds the hits of query
    b by ascending g: idx = index_base + g, val the bits of v; row b is idx[row_ptr[b]:row_ptr[b + 1]].  threshold must be finite;
    the bases >= 0 with index_base + rows <= 2^31 - 1 and query_base + nq <= 2^31 - 1.  With qweight None, v is `search_reference`'s
    value: a row is that search's entries at k = rows with a value >= threshold, by index."""
    q, g = np.asarray(query8), np.asarray(gallery8)
    assert q.ndim == 2 and g.ndim == 2 and q.dtype == np.int8 and g.dtype == np.int8 and q.shape[1] == g.shape[1]
    nq, rows = q.shape[0], g.shape[0]
    threshold = np.float32(threshold)
    if not np.isfinite(threshold):
        raise ValueError("threshold must be finite")
    if index_base < 0 or index_base + rows > 2 ** 31 - 1 or query_base < 0 or query_base + nq > 2 ** 31 - 1:
        raise ValueError("index_base, query_base: >= 0, index_base + rows <= 2^31 - 1 and query_base + nq <= 2^31 - 1")
    v = (q.astype(np.int32) @ g.astype(np.int32).T).astype(np.float32)
    if weight is not None:
        weight = np.asarray(weight, dtype=np.float32)
        assert weight.shape == (rows,)
        v = v * weight[None, :]                                       # one float32 multiply
    if qweight is not None:
        qweight = np.asarray(qweight, dtype=np.float32)
        assert qweight.shape == (nq,)
        v = v * qweight[:, None]                                      # and the second
    assert v.dtype == np.float32
    hit = v >= threshold
    if triangle:
        hit &= (index_base + np.arange(rows, dtype=np.int64))[None, :] > (query_base + np.arange(nq, dtype=np.int64))[:, None]
    row_ptr = np.zeros(nq + 1, np.int64)
    np.cumsum(hit.sum(axis=1), out=row_ptr[1:])
    b, c = np.nonzero(hit)                                            # row-major: by query, then by ascending g
    return row_ptr, (c + index_base).astype(np.int32), v[b, c]


def _images_of(item, transform):
    images = item[0] if isinstance(item, (tuple, list)) else item
    return images if transform is None else transform(images)


def embed8(engine, batches, transform=None):
    """`embed`'s loop keeping the integers: every batch is one engine.features(images) — no head GEMM — and its int8 rows are kept
    (a copy: the engine reuses its buffers), in order.  Nothing inside the loop synchronises.  Returns (feat8 int8
    [N, num_features] on the engine's device, scale): the integers the head reads and their scale (`feature_scale_host()`), what
    `ivit_amd.search.Gallery` takes."""
    rows = [torch.as_tensor(engine.features(_images_of(item, transform))[0]).clone() for item in batches]
    scale = float(engine.feature_scale_host())
    if not rows:
        return torch.zeros(0, int(engine.num_features), dtype=torch.int8, device=getattr(engine, "device", "cpu")), scale
    return torch.cat(rows), scale


def knn_evaluate(engine, gallery, batches, k=20, T=0.07, topk=(1, 5), transform=None):
    """`evaluate`'s loop and return dict with the weighted k-NN vote in place of the head: `batches` yields (images, labels);
    every batch is one engine.retrieve(images, gallery, k) and one `search.knn_classify` of its neighbours against
    `gallery.labels` (cosines: the query's inverse norm is applied to a cosine gallery's values), and counts, for every j of `topk`,
    the images whose label is among the first j classes of the vote.  The hit counts stay on the device until the loop ends.
    Returns {"n": images, "correct": {j: count}, "acc": {j: 100 * count / n}}."""
    from .search import knn_classify, query_inv_norms
    topk = tuple(int(j) for j in topk)
    if not topk or min(topk) < 1:
        raise ValueError("topk must name ranks >= 1")
    if gallery.labels is None:
        raise ValueError("knn_evaluate needs a gallery with labels")
    kk = min(max(topk), int(gallery.num_classes))
    n, hits = 0, None
    for images, labels in batches:
        if transform is not None:
            images = transform(images)
        idx, val, feat8 = engine.retrieve(images, gallery, k=k)
        order, _ = knn_classify(idx, val, gallery.labels, gallery.num_classes, T=T,
                                query_inv_norm=query_inv_norms(feat8) if gallery.cosine else None)
        labels = torch.as_tensor(labels).to(device=order.device, dtype=torch.int64, non_blocking=True).reshape(-1, 1)
        within = (order[:, :kk] == labels).cumsum(1) > 0
        step = torch.stack([within[:, min(j, kk) - 1].sum() for j in topk])
        hits = step if hits is None else hits + step
        n += order.shape[0]
    if hits is None:
        hits = torch.zeros(len(topk), dtype=torch.int64, device=getattr(engine, "device", "cpu"))
    c = [int(v) for v in hits.cpu().tolist()]
    correct = {j: c[t] for t, j in enumerate(topk)}
    return {"n": n, "correct": correct, "acc": {j: (100.0 * v / n if n else float("nan")) for j, v in correct.items()}}


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


def evaluate(engine, batches, topk=(1, 5), transform=None, rank=0, world=1, loss=False, views=1):
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
    plus "loss": loss_sum / n, the reference's `Loss` (NaN if a label lies outside the classes).

    views=V > 1 (five-crop, ten-crop: ivit_amd/views.py): `transform` yields B * V images for the B labels of a batch, the V views
    of an image in consecutive rows, and the loop calls engine.predict_views / engine.score_views instead — predictions and loss
    of the MEAN logits of every image's views.  n counts images, not views.  views=1 is the path above, unchanged."""
    topk = tuple(int(j) for j in topk)
    if not topk or min(topk) < 1:
        raise ValueError("topk must name ranks >= 1")
    views = int(views)
    if not 1 <= views <= MAX_VIEWS:
        raise ValueError(f"views = {views} outside 1 .. {MAX_VIEWS}")
    if loss:
        return _evaluate_with_loss(engine, batches, topk, transform, rank, world, views)
    k = min(max(topk), int(engine.cfg.num_classes))
    n, hits = 0, None                                                   # hits[t]: images whose label is among the first topk[t]
    for images, labels in batches:
        if transform is not None:
            images = transform(images)
        idx = torch.as_tensor(engine.predict(images, k=k)[0] if views == 1 else engine.predict_views(images, views=views, k=k)[0])
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


def _evaluate_with_loss(engine, batches, topk, transform, rank, world, views=1):
    """evaluate(loss=True): see there"""
    n, sums = 0, None                                                   # sums: [hits of topk[0], ..., loss_sum] in float64
    for images, labels in batches:
        if transform is not None:
            images = transform(images)
        device = getattr(engine, "device", "cpu")
        labels = torch.as_tensor(labels).to(device=device, dtype=torch.int64, non_blocking=True).reshape(-1)
        rk, nll = (torch.as_tensor(t) for t in (engine.score(images, labels) if views == 1 else engine.score_views(images, labels, views=views)))
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


# ---------------------------------------------------------------- linear probe (include/ivit_probe.h, ivit_amd/probe.py)
def probe_stats_reference(feat8, labels, num_classes):
    """feat8 int8 [rows, dim], labels integers [rows] -> (gram int64 [dim, dim], class_sum int64 [num_classes, dim], count int64
    [num_classes]): the statistics `ivit_probe_accumulate` ADDS into its buffers.  Row r takes part iff 0 <= labels[r] < num_classes
    (as int64: 2^32 + 3 is no class); gram = X^T X over those rows, class_sum[c] the sum of class c's rows, count[c] their number.
    Exact integers."""
    x, lab = np.asarray(feat8), np.asarray(labels).astype(np.int64).reshape(-1)
    assert x.ndim == 2 and x.dtype == np.int8 and lab.shape == (x.shape[0],)
    C = int(num_classes)
    keep = (lab >= 0) & (lab < C)
    x, lab = x[keep].astype(np.int64), lab[keep]
    gram = x.T @ x
    class_sum = np.zeros((C, x.shape[1]), np.int64)
    np.add.at(class_sum, lab, x)
    count = np.bincount(lab, minlength=C).astype(np.int64)
    return gram, class_sum, count


def probe_system(gram, class_sum, count, ridge=1e-3):
    """the linear system of the ridge probe from the statistics, float64 throughout -> (A [dim, dim], M [C, dim], mu [dim], n):
        n = sum(count);  mu = sum_c class_sum[c] / n;  Gc = gram / n - mu mu^T;  M[c] = class_sum[c] / n - (count[c] / n) mu
        A = Gc + ridge * (trace(Gc) / dim) * I
    Gc is the features' covariance, M[c] the covariance of the features with class c's indicator; the ridge is relative to the mean
    feature variance, so one value serves every model."""
    gram, class_sum, count = (np.asarray(a).astype(np.float64) for a in (gram, class_sum, count))
    dim = gram.shape[0]
    n = count.sum()
    if not n > 0:
        raise ValueError("the statistics hold no row")
    mu = class_sum.sum(axis=0) / n
    Gc = gram / n - np.outer(mu, mu)
    M = class_sum / n - np.outer(count / n, mu)
    A = Gc + float(ridge) * (np.trace(Gc) / dim) * np.eye(dim)
    return A, M, mu, n


def probe_fit_reference(gram, class_sum, count, ridge=1e-3):
    """the statistics -> (V float64 [C, dim], b float64 [C]): V = solve(A, M^T)^T and b[c] = count[c] / n - V[c] . mu with
    `probe_system`'s A, M, mu, n — the least-squares fit of the classes' indicators on the features' integers x (prediction
    V[c] . x + b[c], on a 0 .. 1 target).  A class with count 0 gets V[c] = 0 and b[c] = 0."""
    A, M, mu, n = probe_system(gram, class_sum, count, ridge)
    cnt = np.asarray(count).astype(np.float64)
    V = np.linalg.solve(A, M.T).T
    b = cnt / n - V @ mu
    empty = cnt == 0
    V[empty] = 0.0
    b[empty] = 0.0
    return V, b


def probe_fit(engine, batches, num_classes, ridge=1e-3, transform=None, stats=None):
    """`embed`'s loop over (images, labels) ending in `probe.fit`: every batch is one engine.probe_accumulate — `features` without the
    head, then ivit_probe_accumulate on the same stream; no feature is kept and nothing inside the loop synchronises.  Returns the
    Head for `engine.with_head`.  `stats`: the caller's own ProbeStats to add into — it then holds the statistics afterwards, from
    which `probe.fit` refits with another ridge without a second pass."""
    from .probe import ProbeStats, fit
    if stats is None:
        stats = ProbeStats(engine.num_features, num_classes, engine.device)
    for images, labels in batches:
        if transform is not None:
            images = transform(images)
        labels = torch.as_tensor(labels).to(device=engine.device, dtype=torch.int64, non_blocking=True).reshape(-1)
        engine.probe_accumulate(images, labels, stats)
    return fit(stats, engine.feature_scale_host(), ridge)


# ---------------------------------------------------------------- k-means (include/ivit_cluster.h, ivit_amd/cluster.py)
KMEANS_MAX_K = 16384   # KMEANS_MAX_K of csrc/ivit_cluster.h


def kmeans_norms_reference(cent8):
    """cent8 int8 [K, dim] -> int32 [K]: cnorm[j] = sum_c cent[j, c]^2, exact (at most 2^24 for dim <= 1024)"""
    c = np.asarray(cent8)
    assert c.ndim == 2 and c.dtype == np.int8
    return (c.astype(np.int32) ** 2).sum(axis=1).astype(np.int32)


def kmeans_assign_reference(x8, cent8):
    """x8 int8 [rows, dim], cent8 int8 [K, dim] -> (assign int32 [rows], dist2 int32 [rows]), what `ivit_kmeans_assign` writes.
    s[r, j] = 2 dot[r, j] - cnorm[j] with dot the exact int32 product (|s| <= 2^26); assign[r] is the SMALLEST j that maximises
    s[r, j] (np.argmax returns the first): the nearest centroid in squared Euclidean distance, ties to the lower index;
    dist2[r] = sum_c x[r, c]^2 - s[r, assign[r]], the exact squared distance."""
    x, c = np.asarray(x8), np.asarray(cent8)
    assert x.ndim == 2 and c.ndim == 2 and x.dtype == np.int8 and c.dtype == np.int8 and x.shape[1] == c.shape[1] and c.shape[0] >= 1
    cn = kmeans_norms_reference(c)
    xx = (x.astype(np.int32) ** 2).sum(axis=1)
    assign, dist2 = np.zeros(x.shape[0], np.int32), np.zeros(x.shape[0], np.int32)
    c32 = c.astype(np.int32).T
    for a in range(0, x.shape[0], 4096):                               # pieces: the [rows, K] matrix is never whole
        s = 2 * (x[a:a + 4096].astype(np.int32) @ c32) - cn[None, :]
        j = np.argmax(s, axis=1)
        assign[a:a + 4096] = j
        dist2[a:a + 4096] = xx[a:a + 4096] - s[np.arange(len(j)), j]
    return assign, dist2


def kmeans_stats_reference(x8, assign, dist2, K):
    """x8 int8 [rows, dim], assign integers [rows], dist2 integers [rows] or None -> (sum int64 [K, dim], count int64 [K], inertia
    int64 scalar): what `ivit_kmeans_accumulate` ADDS into its buffers.  Row r takes part iff 0 <= assign[r] < K; with dist2 None
    the inertia is 0 (the entry leaves its buffer untouched)."""
    x, a = np.asarray(x8), np.asarray(assign).astype(np.int64).reshape(-1)
    assert x.ndim == 2 and x.dtype == np.int8 and a.shape == (x.shape[0],)
    K = int(K)
    keep = (a >= 0) & (a < K)
    total = np.zeros((K, x.shape[1]), np.int64)
    np.add.at(total, a[keep], x[keep].astype(np.int64))
    count = np.bincount(a[keep], minlength=K).astype(np.int64)
    inertia = np.int64(0) if dist2 is None else np.asarray(dist2).astype(np.int64).reshape(-1)[keep].sum(dtype=np.int64)
    return total, count, inertia


def kmeans_update_reference(total, count, cent8):
    """sum int64 [K, dim], count int64 [K], cent8 int8 [K, dim] -> (cent' int8 [K, dim], cnorm' int32 [K], moved): what
    `ivit_kmeans_update` leaves.  For every j with count[j] > 0: cent'[j, c] = (2 sum[j, c] + count[j]) // (2 count[j]) — floor
    division: the mean rounded half up, always in -128 .. 127 for sums of int8 rows; an empty cluster keeps its centroid.  moved is the
    number of centroids of which any byte changed."""
    total, count, c = np.asarray(total).astype(np.int64), np.asarray(count).astype(np.int64), np.asarray(cent8)
    assert c.dtype == np.int8 and total.shape == c.shape and count.shape == (c.shape[0],)
    live = count > 0
    n = np.where(live, count, 1)[:, None]
    new = np.where(live[:, None], (2 * total + n) // (2 * n), c.astype(np.int64))
    assert new.min(initial=0) >= -128 and new.max(initial=0) <= 127, "a mean outside int8: the sums are no sums of int8 rows"
    new = new.astype(np.int8)
    return new, kmeans_norms_reference(new), int((new != c).any(axis=1).sum())


def kmeans_reference(x8, cent0, iters):
    """`iters` Lloyd iterations from cent0 -> (cent int8 [K, dim], assign int32 [rows], inertia [iters] int64): every iteration is
    assign (against the centroids it starts with), stats, update; `assign` and inertia[i] are those of iteration i's assignment,
    the centroids those after the last update.  Rounding the mean to int8 means the inertia need not fall monotonically."""
    cent = np.asarray(cent0).copy()
    assign, history = np.zeros(np.asarray(x8).shape[0], np.int32), []
    for _ in range(int(iters)):
        assign, dist2 = kmeans_assign_reference(x8, cent)
        total, count, inertia = kmeans_stats_reference(x8, assign, dist2, cent.shape[0])
        cent, _, _ = kmeans_update_reference(total, count, cent)
        history.append(int(inertia))
    return cent, assign, np.asarray(history, np.int64)


def kmeans_fit(engine, batches, K, iters=20, init="kmeans++", generator=None, transform=None):
    """`embed8` followed by `cluster.KMeans.fit`: the int8 features of the whole dataset are kept on the device (rows x num_features
    bytes), the centroids seeded on the host by `init` ("sample" or "kmeans++") with `generator` (default: np.random.default_rng(0)),
    then `iters` Lloyd iterations of three launches each.  Returns (kmeans, feat8, inertia_history)."""
    from .cluster import KMeans
    feat8, _ = embed8(engine, batches, transform)
    km = KMeans(int(K), int(engine.num_features), feat8.device)
    km.init(feat8, method=init, generator=generator)
    return km, feat8, km.fit(feat8, iters=iters)


def find_duplicates(engine, batches, threshold, transform=None):
    """`embed8`'s loop followed by `search.duplicates`: every pair i < j of the images `batches` yields whose cosine, as
    `range_reference` states it on the int8 features, is >= threshold.  Returns (pairs int64 [P, 2], val float32 [P], feat8)."""
    from .search import duplicates
    feat8, _ = embed8(engine, batches, transform)
    pairs, val = duplicates(feat8, threshold, cosine=True)
    return pairs, val, feat8
