"""Linear probe on a frozen backbone (include/ivit_probe.h): `ProbeStats` holds the three exact integer statistics of the training
features on the device and takes batches through `ivit_probe_accumulate`; `fit` solves the least-squares (ridge) probe from them in
float64 on the host; `Head` is a float head quantised by the reference's QuantLinear rule on the features' scale — what
`engine.with_head` puts into an engine in place of the head it was frozen with.  The numpy statements are
`predict.probe_stats_reference` and `predict.probe_fit_reference`.  torch is used for device memory and streams only: the fit and
the quantisation are numpy."""
import ctypes

import numpy as np
import torch

from . import _lib
from .freeze import quantize_bias, quantize_weight

_P = ctypes.c_void_p
MIN_DIM, MAX_DIM, MAX_CLASSES = 64, 1024, 65536          # PROBE_MIN_DIM, PROBE_MAX_DIM, PROBE_MAX_CLASSES of csrc/ivit_probe.h


class ProbeStats:
    """ProbeStats(dim, num_classes, device): gram int64 [dim, dim], class_sum int64 [num_classes, dim], count int64 [num_classes],
    zeroed tensors on `device` — the whole state of a probe's training pass (dim^2 + C dim + C 64-bit words, whatever the number of
    images).  `add` needs a HIP device; `merge`, `numpy`, `zero_` and `all_reduce` work on any (the host too: what a gloo rank
    holds)."""

    def __init__(self, dim, num_classes, device="cuda:0"):
        dim, num_classes = int(dim), int(num_classes)
        if dim % 64 or not MIN_DIM <= dim <= MAX_DIM:
            raise ValueError(f"dim = {dim}: a multiple of 64 in {MIN_DIM} .. {MAX_DIM}")
        if not 1 <= num_classes <= MAX_CLASSES:
            raise ValueError(f"num_classes = {num_classes} outside 1 .. {MAX_CLASSES}")
        self.dim, self.num_classes, self.device = dim, num_classes, torch.device(device)
        self.gram = torch.zeros(dim, dim, dtype=torch.int64, device=self.device)
        self.class_sum = torch.zeros(num_classes, dim, dtype=torch.int64, device=self.device)
        self.count = torch.zeros(num_classes, dtype=torch.int64, device=self.device)
        self.h = None

    @classmethod
    def from_numpy(cls, gram, class_sum, count, device="cpu"):
        """the statistics of a numpy triple (`predict.probe_stats_reference`, a saved `numpy()`) on `device`"""
        class_sum = np.asarray(class_sum)
        out = cls(class_sum.shape[1], class_sum.shape[0], device)
        for t, a in ((out.gram, gram), (out.class_sum, class_sum), (out.count, count)):
            a = np.ascontiguousarray(a, np.int64)
            if tuple(a.shape) != tuple(t.shape):
                raise ValueError(f"shape {a.shape}, expected {tuple(t.shape)}")
            t.copy_(torch.from_numpy(a))
        return out

    def add(self, feat8, labels, splits=0):
        """feat8 int8 device tensor [rows, dim], labels int64 device tensor [rows]: one ivit_probe_accumulate on the current stream,
        nothing synchronised.  A row whose label is outside 0 .. num_classes - 1 is ignored.  Returns self."""
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise _lib.IvitError("ProbeStats.add needs a HIP device; the product path has no CPU fallback")
        assert isinstance(feat8, torch.Tensor) and feat8.dtype == torch.int8 and feat8.is_contiguous() and feat8.device == self.device
        assert feat8.dim() == 2 and feat8.shape[1] == self.dim, f"feat8 must be [rows, {self.dim}]"
        assert isinstance(labels, torch.Tensor) and labels.dtype == torch.int64 and labels.is_contiguous() and labels.device == self.device
        assert labels.shape == (feat8.shape[0],), f"labels must be [{feat8.shape[0]}]"
        if feat8.shape[0] == 0:                          # an empty batch (an empty shard): nothing to add, and torch gives it no address
            return self
        if self.h is None:
            dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
            self.h = _lib.Handle(dev_index, torch.cuda.current_stream(self.device).cuda_stream)
        self.h.set_stream(torch.cuda.current_stream(self.device).cuda_stream)
        self.h.call("ivit_probe_accumulate", _P(feat8.data_ptr()), _P(labels.data_ptr()), int(feat8.shape[0]), self.dim, self.num_classes,
                    int(splits), _P(self.gram.data_ptr()), _P(self.class_sum.data_ptr()), _P(self.count.data_ptr()))
        return self

    def merge(self, other):
        """adds the statistics of another ProbeStats (or a numpy triple) of the same shape; returns self"""
        g, s, c = other.tensors() if isinstance(other, ProbeStats) else (torch.from_numpy(np.ascontiguousarray(a, np.int64)) for a in other)
        if tuple(g.shape) != tuple(self.gram.shape) or tuple(s.shape) != tuple(self.class_sum.shape) or tuple(c.shape) != tuple(self.count.shape):
            raise ValueError("merge: the statistics have another dim or num_classes")
        self.gram += g.to(self.device)
        self.class_sum += s.to(self.device)
        self.count += c.to(self.device)
        return self

    def tensors(self):
        return self.gram, self.class_sum, self.count

    def all_reduce(self):
        """one all-reduce (sum) of the three tensors over the initialised process group, as ONE int64 tensor; integers: every rank
        ends with the same bits, whatever the order.  gloo reduces host tensors.  Returns self."""
        import torch.distributed as dist
        if not dist.is_initialized():
            raise RuntimeError("ProbeStats.all_reduce needs an initialised process group")
        flat = torch.cat([t.reshape(-1) for t in self.tensors()])
        if dist.get_backend() == "gloo":
            flat = flat.cpu()
        dist.all_reduce(flat, op=dist.ReduceOp.SUM)
        o = 0
        for t in self.tensors():
            t.copy_(flat[o:o + t.numel()].reshape(t.shape))
            o += t.numel()
        return self

    def numpy(self):
        """(gram, class_sum, count) as int64 numpy arrays (synchronises)"""
        return tuple(t.cpu().numpy() for t in self.tensors())

    def zero_(self):
        for t in self.tensors():
            t.zero_()
        return self


class Head:
    """An int8 classification head on a backbone's features: what the reference's `head` (a QuantLinear behind qact2 / qact3) holds
    once frozen.  weight float32 [C, dim] and bias float32 [C] are what one would load into the reference's head; w8 int8 [C, dim],
    weight_scale float32 [C], b32 int32 [C] and scale float32 [C] = fl32(weight_scale * feature_scale) their quantised form
    (freeze.quantize_weight / quantize_bias); a logit times its class's scale is the float output."""

    def __init__(self, weight, bias, feature_scale, w8, weight_scale, b32, scale):
        self.weight, self.bias, self.feature_scale = weight, bias, float(np.float32(feature_scale))
        self.w8, self.weight_scale, self.b32, self.scale = w8, weight_scale, b32, scale

    @property
    def num_classes(self):
        return int(self.w8.shape[0])

    @property
    def dim(self):
        return int(self.w8.shape[1])

    @classmethod
    def from_float(cls, weight, bias, feature_scale):
        """weight [C, dim] float32, bias [C] float32, feature_scale the scale of the features' integers: the reference's QuantLinear
        on a float head whose input scale is the features'.  OverflowError where a bias does not fit int32."""
        weight = np.ascontiguousarray(weight, np.float32)
        bias = np.ascontiguousarray(bias, np.float32)
        if weight.ndim != 2 or bias.shape != (weight.shape[0],):
            raise ValueError("weight [C, dim] and bias [C]")
        w8, weight_scale = quantize_weight(weight)
        b32, scale = quantize_bias(bias, weight_scale, feature_scale)
        return cls(weight, bias, feature_scale, w8, weight_scale, b32, scale)

    def logits_reference(self, feat8):
        """feat8 int8 [B, dim] -> int32 [B, C]: w8 . feat8 + b32, the head's accumulators (what `forward` returns)"""
        f = np.asarray(feat8)
        assert f.ndim == 2 and f.dtype == np.int8 and f.shape[1] == self.dim
        acc = f.astype(np.int64) @ self.w8.astype(np.int64).T + self.b32.astype(np.int64)[None, :]
        assert np.all(np.abs(acc) < 2 ** 31), "a logit does not fit int32"
        return acc.astype(np.int32)


def fit(stats, feature_scale, ridge=1e-3):
    """stats a ProbeStats or a numpy triple (gram, class_sum, count), feature_scale the scale of the features' integers -> Head: the
    least-squares probe on one-hot targets with a ridge relative to the mean feature variance, as `predict.probe_fit_reference`
    states it (float64 throughout, a dim x dim solve on the host), then `Head.from_float(fl32(V / feature_scale), fl32(b),
    feature_scale)`: V acts on the integers, the float head on integers * feature_scale."""
    from .predict import probe_fit_reference
    gram, class_sum, count = stats.numpy() if isinstance(stats, ProbeStats) else stats
    V, b = probe_fit_reference(gram, class_sum, count, ridge)
    s = np.float64(np.float32(feature_scale))
    return Head.from_float((V / s).astype(np.float32), b.astype(np.float32), feature_scale)
