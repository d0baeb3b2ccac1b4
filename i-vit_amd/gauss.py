"""Novelty scores on a frozen backbone (include/ivit_gauss.h): the class-conditional Gaussian with a shared covariance over the int8
features — linear discriminant analysis, and the squared Mahalanobis distance to the nearest class mean as the answer to "is this
image like my training data at all?".  `fit` makes a `GaussModel` from the probe's statistics (`probe.ProbeStats`: the Gram matrix, the
class sums and the counts are this model's sufficient statistics) in float64 on the host; `score` is one `ivit_gauss_score` on the
device, which writes neither the whitened rows nor the class scores; `GaussModel.head` is the equal-prior LDA classifier as a `Head`
for `engine.with_head`; `auroc` and `fpr_at_tpr` are the two numbers people quote for a novelty score.  The numpy statements are
`predict.gauss_fit_reference` and `predict.gauss_score_reference`.  torch is used for device memory and streams only."""
import ctypes

import numpy as np
import torch

from . import _lib

_P = ctypes.c_void_p
MIN_DIM, MAX_DIM, MAX_CLASSES, MAX_SPLITS = 64, 1024, 65536, 256     # GAUSS_* of csrc/ivit_gauss.h


class GaussModel:
    """Wh float32 [R, dim], t float32 [R], Wc float32 [C, dim], bc float32 [C] (include/ivit_gauss.h: the definition) and, per
    device, the prepared form `ivit_gauss_score` reads — made by one `ivit_gauss_prepare` on first use and kept."""

    def __init__(self, Wh, t, Wc, bc):
        self.Wh, self.t, self.Wc, self.bc = (np.ascontiguousarray(a, np.float32) for a in (Wh, t, Wc, bc))
        if self.Wh.ndim != 2 or self.Wc.ndim != 2 or self.Wc.shape[1] != self.Wh.shape[1] or self.t.shape != self.Wh.shape[:1] \
                or self.bc.shape != self.Wc.shape[:1]:
            raise ValueError("Wh [R, dim], t [R], Wc [C, dim], bc [C]")
        self.R, self.dim = (int(v) for v in self.Wh.shape)
        self.C = int(self.Wc.shape[0])
        if self.dim % 64 or not MIN_DIM <= self.dim <= MAX_DIM:
            raise ValueError(f"dim = {self.dim}: a multiple of 64 in {MIN_DIM} .. {MAX_DIM}")
        if self.R % 32 or not 32 <= self.R <= self.dim:
            raise ValueError(f"R = {self.R}: a multiple of 32 in 32 .. {self.dim}")
        if not 1 <= self.C <= MAX_CLASSES:
            raise ValueError(f"C = {self.C} outside 1 .. {MAX_CLASSES}")
        self._prepared = {}        # device index -> (Handle, the prepared model: a uint8 device tensor)

    def save(self, path):
        np.savez(path, Wh=self.Wh, t=self.t, Wc=self.Wc, bc=self.bc)

    @classmethod
    def load(cls, path):
        with np.load(path) as f:
            return cls(f["Wh"], f["t"], f["Wc"], f["bc"])

    def prepared(self, device):
        """(Handle, prepared model) on `device`, the handle on that device's current stream; the first call launches
        ivit_gauss_prepare there"""
        device = torch.device(device)
        if device.type != "cuda" or not torch.cuda.is_available():
            raise _lib.IvitError("GaussModel needs a HIP device; the product path has no CPU fallback")
        index = device.index if device.index is not None else torch.cuda.current_device()
        device = torch.device("cuda", index)
        stream = torch.cuda.current_stream(device).cuda_stream
        if index in self._prepared:
            h, model = self._prepared[index]
            h.set_stream(stream)
            return h, model
        nbytes = ctypes.c_size_t(0)
        st = _lib.load().ivit_gauss_model_bytes(self.dim, self.R, self.C, ctypes.byref(nbytes))
        if st != _lib.IVIT_OK:
            raise _lib.IvitError(f"ivit_gauss_model_bytes(dim={self.dim}, R={self.R}, C={self.C}) failed with status {st}")
        h = _lib.Handle(index, stream)
        model = torch.empty(nbytes.value, dtype=torch.uint8, device=device)
        src = [torch.from_numpy(a).to(device) for a in (self.Wh, self.t, self.Wc, self.bc)]
        h.call("ivit_gauss_prepare", *(_P(a.data_ptr()) for a in src), self.dim, self.R, self.C, _P(model.data_ptr()), nbytes.value)
        for a in src:                                    # the launch is queued on `stream`: the allocator may not hand these out before it ran
            a.record_stream(torch.cuda.current_stream(device))
        self._prepared[index] = (h, model)
        return h, model

    def head(self, feature_scale):
        """the equal-prior LDA classifier as a `probe.Head` on the features' scale: argmax_c s[., c] is argmax_c of
        (Wc / 2) . x + bc / 2, and a float head acts on feature_scale * x.  ValueError where a class is empty (bc = -inf)."""
        from .probe import Head
        if not np.isfinite(self.bc).all():
            raise ValueError("the model has an empty class (bc = -inf): a head needs every class")
        s = np.float64(np.float32(feature_scale))
        return Head.from_float((self.Wc.astype(np.float64) / (2.0 * s)).astype(np.float32), (self.bc / 2).astype(np.float32), feature_scale)


def fit(stats, shrinkage=1e-3, rank=None):
    """stats a `probe.ProbeStats` or a numpy triple (gram, class_sum, count) -> GaussModel: `predict.gauss_fit_reference` in float64
    on the host (a dim x dim eigendecomposition), rounded once to float32.  The statistics are exact integers, so a sharded fit is
    `ProbeStats.all_reduce` in front of this."""
    from .predict import gauss_fit_reference
    from .probe import ProbeStats
    gram, class_sum, count = stats.numpy() if isinstance(stats, ProbeStats) else stats
    return GaussModel(*gauss_fit_reference(gram, class_sum, count, shrinkage, rank))


def score(feat8, model, splits=0):
    """feat8 int8 device tensor [N, dim], model a GaussModel -> (dist float32 [N], cls int32 [N], q float32 [N], best float32 [N]),
    device tensors: one ivit_gauss_score on the current stream, nothing synchronised; `predict.gauss_score_reference` is the numpy
    statement.  The results do not depend on `splits`.  The workspace is allocated by torch here (a caller who captures a graph keeps
    the returned tensors)."""
    if not (isinstance(feat8, torch.Tensor) and feat8.is_cuda):
        raise _lib.IvitError("gauss.score needs a HIP device; the product path has no CPU fallback")
    assert feat8.dtype == torch.int8 and feat8.dim() == 2 and feat8.is_contiguous()
    N, dim = (int(v) for v in feat8.shape)
    if dim != model.dim:
        raise _lib.IvitError(f"feat8 is [{N}, {dim}]: the model has {model.dim} features")
    h, prepared = model.prepared(feat8.device)
    nbytes = ctypes.c_size_t(0)
    st = h.lib.ivit_gauss_workspace_bytes(N, dim, model.R, model.C, int(splits), ctypes.byref(nbytes))
    if st != _lib.IVIT_OK:
        raise _lib.IvitError(f"ivit_gauss_workspace_bytes(N={N}, dim={dim}, R={model.R}, C={model.C}, splits={splits}) failed with status {st}")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=feat8.device)
    q, best, dist = (torch.empty(N, dtype=torch.float32, device=feat8.device) for _ in range(3))
    cls = torch.empty(N, dtype=torch.int32, device=feat8.device)
    h.call("ivit_gauss_score", _P(prepared.data_ptr()), prepared.numel(), _P(feat8.data_ptr()), N, dim, model.R, model.C, int(splits),
           _P(ws.data_ptr()), nbytes.value, _P(q.data_ptr()), _P(best.data_ptr()), _P(cls.data_ptr()), _P(dist.data_ptr()))
    return dist, cls, q, best


def auroc(inlier_scores, outlier_scores):
    """the probability that an outlier scores above an inlier (ties count half): the area under the ROC curve of a novelty score
    that is LARGER on outliers.  Host numpy, by ranks."""
    a, b = np.asarray(inlier_scores, np.float64).ravel(), np.asarray(outlier_scores, np.float64).ravel()
    if not len(a) or not len(b):
        raise ValueError("auroc needs at least one score on each side")
    both = np.concatenate([a, b])
    _, inv, cnt = np.unique(both, return_inverse=True, return_counts=True)
    rank = (np.cumsum(cnt) - (cnt - 1) / 2.0)[inv]       # mid-ranks, 1-based
    return float((rank[len(a):].sum() - len(b) * (len(b) + 1) / 2.0) / (len(a) * len(b)))


def fpr_at_tpr(inlier_scores, outlier_scores, tpr=0.95):
    """the fraction of outliers accepted at the threshold that accepts at least `tpr` of the inliers (score <= threshold is
    "inlier"): FPR at 95 % TPR with the inliers as the positive class.  Host numpy."""
    a, b = np.sort(np.asarray(inlier_scores, np.float64).ravel()), np.asarray(outlier_scores, np.float64).ravel()
    if not len(a) or not len(b):
        raise ValueError("fpr_at_tpr needs at least one score on each side")
    thr = a[min(len(a) - 1, max(0, int(np.ceil(tpr * len(a))) - 1))]
    return float((b <= thr).mean())
