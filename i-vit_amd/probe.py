"""Linear probe on a frozen backbone (include/ivit_probe.h): `ProbeStats` holds the three exact integer statistics of the training
features on the device and takes batches through `ivit_probe_accumulate`; `fit` solves the least-squares (ridge) probe from them in
float64 on the host; `fit_logistic` is multinomial logistic regression by L-BFGS over
`logreg_loss_grad` (include/ivit_logreg.h: the fused loss and gradient on the device); `Head` is a float head quantised by the reference's QuantLinear rule on the features' scale — what
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


# ---------------------------------------------------------------- logistic regression (include/ivit_logreg.h)
_handles = {}          # device index -> the Handle logreg_loss_grad calls through


def logreg_loss_grad(feat8, labels, W, b, x_scale, splits=0):
    """feat8 int8 device tensor [N, dim], labels int32 (or int64: converted) device tensor [N], W float32 [C, dim], b float32 [C] ->
    (loss float64 [1], grad_W float32 [C, dim], grad_b float32 [C], correct int64 [2]), device tensors: one ivit_logreg_loss_grad on
    the current stream, nothing synchronised; `predict.logreg_reference` is the numpy statement.  The workspace is allocated by torch
    here (a caller who captures a graph keeps the returned tensors and calls the C entry itself)."""
    if not (isinstance(feat8, torch.Tensor) and feat8.is_cuda):
        raise _lib.IvitError("logreg_loss_grad needs a HIP device; the product path has no CPU fallback")
    dev = feat8.device
    assert feat8.dtype == torch.int8 and feat8.dim() == 2 and feat8.is_contiguous()
    N, dim = (int(v) for v in feat8.shape)
    labels = labels.to(device=dev, dtype=torch.int32).contiguous()
    W = W.to(device=dev, dtype=torch.float32).contiguous()
    b = b.to(device=dev, dtype=torch.float32).contiguous()
    C = int(W.shape[0])
    assert labels.shape == (N,) and W.shape == (C, dim) and b.shape == (C,)
    nbytes = ctypes.c_size_t(0)
    st = _lib.load().ivit_logreg_workspace_bytes(N, dim, C, int(splits), ctypes.byref(nbytes))
    if st != _lib.IVIT_OK:
        raise _lib.IvitError(f"ivit_logreg_workspace_bytes(N={N}, dim={dim}, C={C}, splits={splits}) failed with status {st}")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    loss = torch.empty(1, dtype=torch.float64, device=dev)
    gW, gb = torch.empty_like(W), torch.empty_like(b)
    correct = torch.empty(2, dtype=torch.int64, device=dev)
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    h = _handles.get(index)
    if h is None:
        h = _handles[index] = _lib.Handle(index, torch.cuda.current_stream(dev).cuda_stream)
    h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    h.call("ivit_logreg_loss_grad", _P(feat8.data_ptr()), _P(labels.data_ptr()), N, dim, _P(W.data_ptr()), _P(b.data_ptr()), C,
           float(x_scale), int(splits), _P(ws.data_ptr()), nbytes.value, _P(loss.data_ptr()), _P(gW.data_ptr()), _P(gb.data_ptr()),
           _P(correct.data_ptr()))
    return loss, gW, gb, correct


def fit_logistic(feat8_or_chunks, labels, num_classes, feature_scale, l2=1e-4, iters=100, tol=1e-6, init=None, evaluate=None):
    """Multinomial logistic regression on int8 features -> Head (through `Head.from_float`): minimises
        f(W, b) = loss / n + (l2 / 2) |W|^2,   loss and n = correct[0] as `ivit_logreg_loss_grad` states them, W acting on
        feature_scale * integers (the head's convention),
    by L-BFGS (history 10) with a backtracking Armijo line search, float64 on the features' device.  Every function evaluation is one
    `logreg_loss_grad` per chunk at fl32(W), fl32(b); the chunks (a list of device tensors, `labels` a matching list or one tensor)
    are summed in list order.  ONE synchronisation per evaluation: the line search reads the scalar objective; nothing else comes to
    the host.  Stops after `iters` iterations, when |grad f| < tol, or when the line search finds no decrease (fp32 weights: the
    objective's last bits).  init=None starts from zeros, init=head (a ridge `Head`) from its float weight and bias.
    `evaluate`: a function with `logreg_loss_grad`'s arguments and results to use in its place (numpy or tensors; the tests pass
    `predict.logreg_reference`).  The result's `fit_info` holds iterations, evaluations, objective, grad_norm and train accuracy."""
    chunks = list(feat8_or_chunks) if isinstance(feat8_or_chunks, (list, tuple)) else [feat8_or_chunks]
    if isinstance(labels, (list, tuple)):
        labs = list(labels)
    else:
        sizes = [int(c.shape[0]) for c in chunks]
        labs = [labels[sum(sizes[:i]):sum(sizes[:i + 1])] for i in range(len(chunks))]
    evaluate = evaluate or logreg_loss_grad
    dev = chunks[0].device if isinstance(chunks[0], torch.Tensor) else torch.device("cpu")
    C, dim, s = int(num_classes), int(chunks[0].shape[1]), float(np.float32(feature_scale))
    theta = torch.zeros(C, dim + 1, dtype=torch.float64, device=dev)
    if init is not None:
        theta[:, :dim] = torch.from_numpy(np.asarray(init.weight, np.float64)).to(dev)
        theta[:, dim] = torch.from_numpy(np.asarray(init.bias, np.float64)).to(dev)
    t64 = lambda a: torch.as_tensor(a).to(device=dev, dtype=torch.float64)
    evals = 0

    def fun(th):
        nonlocal evals
        evals += 1
        W32, b32 = th[:, :dim].float().contiguous(), th[:, dim].float().contiguous()
        loss, g, correct = torch.zeros((), dtype=torch.float64, device=dev), torch.zeros_like(th), torch.zeros(2, dtype=torch.float64, device=dev)
        for x, lab in zip(chunks, labs):
            l, gW, gb, cor = evaluate(x, lab, W32 if isinstance(x, torch.Tensor) else W32.numpy(), b32 if isinstance(x, torch.Tensor) else b32.numpy(), s)
            loss = loss + t64(l).reshape(())
            g[:, :dim] += s * t64(gW)
            g[:, dim] += t64(gb)
            correct = correct + t64(cor)
        n = correct[0].clamp(min=1.0)
        W = W32.double()
        f = loss / n + 0.5 * l2 * (W * W).sum()
        g = g / n
        g[:, :dim] += l2 * W
        return f, g, correct

    f, g, correct = fun(theta)
    S, Y, done = [], [], 0
    for done in range(1, int(iters) + 1):
        gnorm = g.norm()
        q = g.clone()                                    # the two-loop recursion
        alphas = []
        for sv, yv in zip(reversed(S), reversed(Y)):
            a = (sv * q).sum() / (sv * yv).sum()
            alphas.append(a)
            q -= a * yv
        if S:
            q *= (S[-1] * Y[-1]).sum() / (Y[-1] * Y[-1]).sum()
        for (sv, yv), a in zip(zip(S, Y), reversed(alphas)):
            q += (a - (yv * q).sum() / (sv * yv).sum()) * sv
        d = -q
        slope = (g * d).sum()
        f0, step, ok = float(f), 1.0 if S else 1.0 / max(float(gnorm), 1.0), False      # float(): the synchronisation
        if float(gnorm) < tol or not float(slope) < 0:
            done -= 1
            break
        for _ in range(30):                              # Armijo, halving
            fn, gn, cn = fun(theta + step * d)
            if float(fn) <= f0 + 1e-4 * step * float(slope):
                ok = True
                break
            step *= 0.5
        if not ok:
            done -= 1
            break
        sv, yv = step * d, gn - g
        if float((sv * yv).sum()) > 1e-12 * float(sv.norm() * yv.norm()):
            S.append(sv)
            Y.append(yv)
            if len(S) > 10:
                S.pop(0)
                Y.pop(0)
        theta, f, g, correct = theta + sv, fn, gn, cn
    head = Head.from_float(theta[:, :dim].float().cpu().numpy(), theta[:, dim].float().cpu().numpy(), feature_scale)
    cor = correct.cpu().numpy()
    head.fit_info = {"iterations": done, "evaluations": evals, "objective": float(f), "grad_norm": float(g.norm()),
                     "train_acc": float(cor[1] / max(cor[0], 1.0)), "n": int(cor[0])}
    return head
