"""NativeEngine — what ViTEngine and SwinEngine share: one frozen model behind the C runners of csrc/ivit_model.h.

The base owns the device and handle, the constants blob, the workspace cache and the ways into a runner:
`forward` / `capture` (ivit_<model>_forward, one C call per batch, or its hipGraph), `predict` / `capture_predict` (the same
with the top-k of the dequantised logits behind them, ivit_<model>_predict), `score` / `capture_score` (with the labels' rank and
negative log-likelihood behind them instead, ivit_<model>_score of include/ivit_eval.h) and `features` / `capture_features` (the
reference's forward_features: the integers the head reads and their fp32 form, with or without the head, ivit_<model>_features of
include/ivit_features.h) and `hidden_states` / `capture_hidden_states` (the 16-bit outputs of chosen blocks or stages and their
fp32 form, ivit_<model>_hidden_states of include/ivit_hidden.h); `retrieve` is `features` with a gallery search behind it
(include/ivit_search.h, ivit_amd/search.py), `probe_accumulate` is `features` with the statistics of a linear probe behind it and
`with_head` the way a fitted head comes back as a new engine (include/ivit_probe.h, ivit_amd/probe.py).  Every eager way is its arguments and one `_eager` call, every captured way its arguments and one
`_capture` call; what lives beside a logits buffer (idx / val, rank / nll, feat8 / feat32, a ViT's attn16 / map32) follows the one
rule of `SideOutputs`.  A subclass names its C prefix, builds its parameter structs (`_native_params`), says where its feature
scale lies (`feature_scale_host`, `num_features`) and keeps its `forward_ops`.  torch is used for device memory and streams only.
"""
import ctypes

import numpy as np
import torch

from . import _lib

_P = ctypes.c_void_p


def _ptr(t):
    return _P(t.data_ptr())


def _clone(out):
    """clones of the tensors of a result, tuples of them and None kept as they are"""
    if isinstance(out, tuple):
        return tuple(_clone(t) for t in out)
    return out if out is None else out.clone()


def ascending_indices(indices, n, what):
    """an int or a sequence of indices, negative ones counting from the end -> strictly ascending tuple in [0, n); ValueError
    otherwise.  `what`: what an index names (a block, a stage), for the error texts.  THE rule of every index list an engine takes"""
    seq = (indices,) if isinstance(indices, (int, np.integer)) else tuple(indices)
    if not seq:
        raise ValueError(f"no {what} given")
    out = []
    for b in seq:
        if not isinstance(b, (int, np.integer)) or not -n <= b < n:
            raise ValueError(f"{what} {b!r}: an integer in [-{n}, {n})")
        out.append(int(b) % n)
    if any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError(f"{what}s {seq} -> {tuple(out)}: the indices must be strictly ascending")
    return tuple(out)


class ShapeCache:
    """key -> make(*key), bounded: at most `limit` keys that are not pinned stay resident, the oldest of them leaves first;
    a pinned key never leaves and does not count toward the limit."""

    def __init__(self, make, limit=4):
        self.make, self.limit = make, limit
        self.items, self.pinned = {}, set()

    def __contains__(self, key):
        return key in self.items

    def unpinned(self):
        return [k for k in self.items if k not in self.pinned]

    def pin(self, key):
        self.pinned.add(key)

    def get(self, key):
        if key not in self.items:
            free = self.unpinned()
            if len(free) >= self.limit:
                del self.items[free[0]]
            self.items[key] = self.make(*key)
        return self.items[key]


class SideOutputs:
    """key -> make(), for outputs that live beside a logits buffer of the workspace cache `ws`; key[:2] is that buffer's (batch,
    nslices).  THE rule of every side output: the engine's own, overwritten by the next call of the same key; built again when the
    key is new or its logits buffer is no longer this one (the shape was evicted and rebuilt); before a build every entry that is not
    pinned and whose (batch, nslices) has left `ws` is dropped; a pinned key — a captured graph refers to its tensors — never is."""

    def __init__(self, ws):
        self.ws = ws
        self.items, self.pinned = {}, set()

    def pin(self, key):
        self.pinned.add(key)

    def get(self, key, logits, make):
        hit = self.items.get(key)
        if hit is None or hit[0] is not logits:
            for old in [q for q in self.items if q not in self.pinned and q[:2] not in self.ws]:
                del self.items[old]
            hit = self.items[key] = (logits, make())
        return hit[1]


class NativeEngine:
    # "ivit_vit" / "ivit_swin": the entries are PREFIX + _create, _destroy, _workspace_bytes, _forward, _graph_create, _predict,
    # _predict_graph_create, _score, _score_graph_create, _features and _features_graph_create
    PREFIX = None
    MAX_SLICES = 8

    def __init__(self, cfg, device):
        """refuses without a device; `_load` brings the constants, `_build_native` the model"""
        self.model = None
        if not torch.cuda.is_available():
            raise _lib.IvitError(f"{type(self).__name__} needs a HIP device; the product path has no CPU fallback")
        self.cfg, self.device = cfg, torch.device(device)
        torch.cuda.set_device(self.device)
        # a graph has its buffers baked in: the (batch, slices) shapes one refers to are pinned in the cache (_graph_keys), and
        # _graphs keeps every graph's buffers alive
        self._native_ws = ShapeCache(self._make_buffers)
        self._graph_keys = self._native_ws.pinned
        self._graphs = []
        # (idx, val) per (batch, slices, k); (rank, nll) and (feat8, feat32) per (batch, slices): one SideOutputs per kind
        self._predict_out, self._score_out, self._features_out = (SideOutputs(self._native_ws) for _ in range(3))
        self._hidden_out = SideOutputs(self._native_ws)     # (hid16, hid32, index list) per (batch, slices, sites, layout)
        # views (include/ivit_views.h): (sum, idx, val) per (groups, k), (sum, rank, nll) per (groups, 0); the scale vector per V
        self._views_out = ShapeCache(self._make_view_buffers)
        self._view_scale = {}
        self._gstream = None                    # the stream graphs are captured and replayed on, made by the first capture
        self._head_scale_host = None
        self._input_scale = None                # the scale of qact_input, where the engine was told (input_scale_host)
        self.last_logits = None

    def _load(self, blob, table):
        """the packed constants (host numpy blob, or a uint8 tensor from a broadcast) onto the device, and the handle on the
        current stream"""
        self.table = table
        self.blob = torch.from_numpy(blob).to(self.device) if isinstance(blob, np.ndarray) else blob.to(self.device)
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.h = _lib.Handle(dev_index, torch.cuda.current_stream(self.device).cuda_stream)

    def ptr(self, name):
        return _P(self.blob.data_ptr() + self.table[name][0])

    def head_scale_host(self):
        """host float32 copy [num_classes] of the head's scale (the reference's head.bias_scaling_factor), read from the device
        once; every call returns a fresh array, the caller's to change."""
        if self._head_scale_host is None:
            o, _, shp = self.table["head.scale"]
            self._head_scale_host = self.blob[o:o + 4 * int(np.prod(shp))].cpu().numpy().view(np.float32).copy()
        return self._head_scale_host.copy()

    def input_scale_host(self):
        """host float: the scale the int8 images are quantised at (the reference's qact_input), for an engine built from scales or
        loaded from a model file; IvitError for an engine that was never told (built from a broadcast package without
        input_scale=)"""
        if self._input_scale is None:
            raise _lib.IvitError("this engine was never told its input scale: build it from scales, load it from a model file, or pass "
                                 "input_scale= to the constructor")
        return self._input_scale

    def _file_package(self):
        """(kind, scalars without "input.s", extras) of model_file.write for this engine"""
        raise NotImplementedError

    def save(self, path):
        """the engine as a model file (include/ivit_modelfile.h, ivit_amd.model_file): the configuration, the constants blob as it
        lies in device memory, the host scalars, the input scale — what `ivit_amd.load_engine` and the C library's
        `ivit_model_open` read.  Returns `path`.  IvitError where the engine lacks what a file must hold (the input scale, the
        features' scale, a Swin's class_scale)."""
        from . import model_file
        kind, scalars, extras = self._file_package()
        scalars = dict(scalars, **{"input.s": ("f", float(np.float32(self.input_scale_host())))})
        return model_file.write(path, kind, self.cfg, self.blob.cpu().numpy(), self.table, scalars, extras)

    def _entry(self, suffix, *args):
        name = self.PREFIX + suffix
        self.h._check(getattr(self.h.lib, name)(*args), name)

    def _native_params(self):
        """(config struct, params struct, keep-alive) of PREFIX_create"""
        raise NotImplementedError

    def _build_native(self):
        """PREFIX_create: hand the runner device pointers into the blob + host scalars."""
        c, prm, self._native_keep = self._native_params()
        model = _P()
        self._entry("_create", self.h.h, ctypes.byref(c), ctypes.byref(prm), self.MAX_SLICES, ctypes.byref(model))
        self.model = model

    def __del__(self):
        try:
            if self.model:
                getattr(self.h.lib, self.PREFIX + "_destroy")(self.model)
                self.model = None
        except Exception:
            pass

    def _workspace_init(self, ws, B, nslices):
        """what a fresh workspace needs before its first forward: nothing, unless the subclass says"""

    def _make_buffers(self, B, nslices):
        n = ctypes.c_size_t()
        self._entry("_workspace_bytes", self.model, B, nslices, ctypes.byref(n))
        ws = torch.empty(n.value, dtype=torch.uint8, device=self.device)
        logits = torch.empty(B, self.cfg.num_classes, dtype=torch.int32, device=self.device)
        self._workspace_init(ws, B, nslices)
        return ws, logits

    def _native_buffers(self, B, nslices):
        """(workspace, logits) of one (batch, slices), the engine's own: see ShapeCache"""
        return self._native_ws.get((B, nslices))

    def _empty(self, dtype, *shape):
        return torch.empty(*shape, dtype=dtype, device=self.device)

    def _check_labels(self, labels, B):
        assert isinstance(labels, torch.Tensor) and labels.dtype == torch.int64 and labels.device == self.device, "labels: int64 device tensor"
        assert labels.shape == (B,) and labels.is_contiguous(), f"labels must be a contiguous [{B}]"

    def _score_args(self, images, labels, nslices):
        """(arguments of the score entries, cache key, buffers) for one batch and its labels"""
        B = images.shape[0]
        self._check_labels(labels, B)
        args, key, (ws, logits) = self._args(images, nslices)
        rank, nll = self._score_out.get(key, logits, lambda: (self._empty(torch.int32, B), self._empty(torch.float64, B)))
        return args + (self.ptr("head.scale"), _ptr(labels), _ptr(rank), _ptr(nll)), key, (ws, logits, rank, nll)

    @property
    def num_features(self):
        """width of a features row: embed_dim of a ViT, embed_dim << (num_layers - 1) of a Swin"""
        raise NotImplementedError

    def feature_scale_host(self):
        """host float: the scale of the features' integers (the reference's qact2 of a ViT, qact3 of a Swin)"""
        raise NotImplementedError

    def _features_args(self, images, normalize, logits, nslices):
        """(arguments of the features entries, cache key, buffers) for one batch; without `logits` the head's pointer is NULL"""
        args, key, (ws, lg) = self._args(images, nslices)
        shape = (images.shape[0], self.num_features)
        feat8, feat32 = self._features_out.get(key, lg, lambda: (self._empty(torch.int8, *shape), self._empty(torch.float32, *shape)))
        mode = _lib.IVIT_FEATURES_UNIT if normalize else _lib.IVIT_FEATURES_DEQUANT
        return (args[:-1] + (_ptr(lg) if logits else None, _ptr(feat8), float(self.feature_scale_host()), mode, _ptr(feat32)), key,
                (ws, lg, feat8, feat32))

    # ---- hidden states (include/ivit_hidden.h): the outputs of chosen blocks (ViT) or stages (Swin).  A subclass says how many sites
    # it has, what a plane looks like and whether row 0 is a class token
    HIDDEN_CLASS_ROW = False        # True: the grid form drops row 0 of every plane
    HIDDEN_SITE = "site"            # what an index names, for the error texts

    def _hidden_sites(self):
        """number of sites: depth of a ViT, num_layers of a Swin"""
        raise NotImplementedError

    def _hidden_plane(self, i):
        """(tokens, width, grid side) of site i's output"""
        raise NotImplementedError

    def _hidden_views(self, hid16, hid32, planes, B, layout):
        """what the caller gets for the packed buffers: per-model views"""
        raise NotImplementedError

    def hidden_scale_host(self, i):
        """host float: the per-tensor scale of site i's output (the reference's blocks.{i}.qact4 of a ViT, that of the last block
        of stage i of a Swin), as the native model holds it; negative indices count from the end"""
        n = self._hidden_sites()
        if not isinstance(i, (int, np.integer)) or not -n <= i < n:
            raise ValueError(f"{self.HIDDEN_SITE} {i!r}: an integer in [-{n}, {n})")
        s = ctypes.c_float()
        self._entry("_hidden_scale", self.model, int(i) % n, ctypes.byref(s))
        return float(s.value)

    def _hidden_list(self, sites):
        return ascending_indices(sites, self._hidden_sites(), self.HIDDEN_SITE)

    def _hidden_args(self, images, sites, layout, logits, nslices):
        """(arguments of the hidden_states entries, cache key, buffers, what the caller gets) for one batch: hid16 and hid32 are
        packed plane after plane, live beside the logits buffer and follow its rule (SideOutputs)"""
        sites = self._hidden_list(sites)
        if layout not in (None, "tokens", "grid"):
            raise ValueError(f"layout = {layout!r}: None, 'tokens' or 'grid'")
        args, key, (ws, lg) = self._args(images, nslices)
        B, n = images.shape[0], len(sites)
        planes = [self._hidden_plane(i) for i in sites]
        t0 = 1 if (self.HIDDEN_CLASS_ROW and layout == "grid") else 0
        n16, n32 = sum(B * T * C for T, C, _ in planes), sum(B * (T - t0) * C for T, C, _ in planes)
        okey = key + (sites, layout)
        hid16, hid32, host = self._hidden_out.get(okey, lg, lambda: (
            self._empty(torch.int16, n16), None if layout is None else self._empty(torch.float32, n32), (ctypes.c_int * n)(*sites)))
        mode = _lib.IVIT_HIDDEN_GRID if layout == "grid" else _lib.IVIT_HIDDEN_TOKENS
        args = args[:-1] + (_ptr(lg) if logits else None, host, n, _ptr(hid16), mode, None if hid32 is None else _ptr(hid32))
        out = self._hidden_views(hid16, hid32, planes, B, layout) + ((lg,) if logits else ())
        return args, okey, (ws, lg, hid16, hid32, host), out

    def hidden_states(self, images, sites=-1, layout=None, logits=False, nslices=1, copy=False):
        """images int8 [B, C, H, W] -> (hid16, hid32), or (hid16, hid32, logits) with logits=True: the 16-bit outputs of the sites
        asked for (an int or a sequence; negative indices count from the end; strictly ascending after that, else ValueError) — the
        integers of the reference's closing QuantAct of a block, qact4, whose scale is `hidden_scale_host(i)` — and, with layout
        "tokens" or "grid", their fp32 form as `predict.hidden_reference` states it (None with layout=None).  One native call: the
        last launch of a tapped block writes the caller's plane, no copy; one launch per plane for the fp32 form.  Without `logits`
        the forward ends behind the last site asked for; with it the int32 logits are forward's (and `last_logits`).  The results
        are the engine's own buffers for this (batch, nslices, sites, layout): copy=True (or clone) to keep them across calls."""
        def plan():
            args, _, bufs, out = self._hidden_args(images, sites, layout, logits, nslices)
            return args, bufs[1] if logits else None, out
        out = self._eager("_hidden_states", images, False, plan)
        return _clone(out) if copy else out

    def capture_hidden_states(self, images, sites=-1, layout=None, logits=False, nstreams=1):
        """hipGraph of one hidden_states on fixed buffers; returns a callable that replays it and returns what `hidden_states`
        returns.  A replay reads `images` as they are then."""
        self._check_images(images)
        args, okey, bufs, out = self._hidden_args(images, sites, layout, logits, nstreams)
        return self._capture("_hidden_states_graph_create", images, args, okey, tuple(b for b in bufs if b is not None), out, self._hidden_out)

    def _check_images(self, images):
        assert images.dtype == torch.int8 and images.is_contiguous() and images.device == self.device

    def _use_current_stream(self):
        self.h.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    def _args(self, images, nslices, k=None):
        """(arguments of the forward entries — of the predict entries with k —, cache key, buffers) for one batch"""
        B = images.shape[0]
        nslices = max(1, min(int(nslices), B, self.MAX_SLICES))
        ws, logits = bufs = self._native_buffers(B, nslices)
        args = (self.model, _ptr(images), B, nslices, _ptr(ws), ws.numel(), _ptr(logits))
        if k is None:
            return args, (B, nslices), bufs
        key = (B, nslices, int(k))
        idx, val = self._predict_out.get(key, logits, lambda: (self._empty(torch.int32, B, key[2]), self._empty(torch.float32, B, key[2])))
        return args + (self.ptr("head.scale"), key[2], _ptr(idx), _ptr(val)), key, bufs + (idx, val)

    def _eager(self, suffix, images, copy, plan):
        """one call of the entry PREFIX + suffix on the current stream.  `plan()` — an `_args` kind, asked once the stream is set: a
        fresh workspace is initialised on it — gives (C arguments, the logits buffer if the caller is to find it in `last_logits`
        or None, results); returns the results, cloned with `copy`"""
        self._use_current_stream()
        self._check_images(images)
        args, logits, out = plan()
        self._entry(suffix, *args)
        if logits is not None:
            self.last_logits = logits
        return tuple(t.clone() for t in out) if copy else out

    def forward(self, images, nslices=1, copy=False):
        """images: int8 device tensor [B, C, H, W] (already quantised, scale s_in) -> int32 logits
        [B, num_classes] (head accumulators).  One native call; nslices > 1 cuts the batch into slices
        on the runner's internal HIP streams (VALU-bound kernels of one slice share the chip with the
        MFMA-bound GEMMs of another).  Same integers for every nslices.

        The returned tensor is the engine's OWN output buffer for this (batch, nslices): the next forward /
        graph replay of the same shape overwrites it (nothing is allocated per call).  Pass copy=True — or
        clone it — when results of several batches are kept (an eval loop collecting logits)."""
        def plan():
            args, _, (_, logits) = self._args(images, nslices)
            return args, None, (logits,)
        return self._eager("_forward", images, copy, plan)[0]

    def predict(self, images, k=5, nslices=1, copy=False):
        """images int8 [B, C, H, W] -> (idx int32 [B, k], val float32 [B, k]) device tensors: the k best classes of every image in
        the order of `predict.topk_reference`, and their dequantised head outputs.  One native call (the forward, then the top-k
        launch behind the slices' join); the head scale is read where it lies in the constants blob.  The int32 logits of the same
        call are in `last_logits`.  Like forward(), the results are the engine's own buffers for this (batch, nslices, k):
        copy=True (or clone) to keep them across calls.  1 <= k <= min(16, num_classes)."""
        def plan():
            args, _, (_, logits, idx, val) = self._args(images, nslices, k)
            return args, logits, (idx, val)
        return self._eager("_predict", images, copy, plan)

    def score(self, images, labels, nslices=1, copy=False):
        """images int8 [B, C, H, W], labels int64 device tensor [B] -> (rank int32 [B], nll float64 [B]) device tensors: per image
        the number of classes the model puts before the label (the label is among the first j exactly when rank < j) and the
        cross-entropy of the label, as `predict.score_reference` states them.  One native call (the forward, then the score
        launch behind the slices' join); `last_logits` holds the int32 logits of the same call.  The results are the engine's own
        buffers for this (batch, nslices): copy=True (or clone) to keep them across calls."""
        def plan():
            args, _, (_, logits, rank, nll) = self._score_args(images, labels, nslices)
            return args, logits, (rank, nll)
        return self._eager("_score", images, copy, plan)

    def features(self, images, normalize=False, logits=False, nslices=1, copy=False):
        """images int8 [B, C, H, W] -> (feat8 int8 [B, num_features], feat32 float32 [B, num_features]) device tensors, or
        (feat8, feat32, logits) with logits=True: the reference's forward_features.  feat8 holds the integers the head reads (the
        class-token row after norm -> qact2 of a ViT, the pooled row after qact3 of a Swin; their scale is `feature_scale_host()`),
        feat32 their fp32 form as `predict.features_reference` states it: feat8 * scale, the reference's fp32 tensor — or with
        normalize=True the rows at unit Euclidean length.  One native call; without `logits` the head GEMM is not launched, with
        it the int32 logits are forward's (and `last_logits`).  The results are the engine's own buffers for this (batch,
        nslices): copy=True (or clone) to keep them across calls."""
        def plan():
            args, _, (_, lg, feat8, feat32) = self._features_args(images, normalize, logits, nslices)
            return args, lg if logits else None, (feat8, feat32) + ((lg,) if logits else ())
        return self._eager("_features", images, copy, plan)

    def retrieve(self, images, gallery, k=20, nslices=1, copy=False):
        """images int8 [B, C, H, W], gallery an `ivit_amd.search.Gallery` of this backbone's features -> (idx int32 [B, k], val
        float32 [B, k], feat8 int8 [B, num_features]) device tensors: `features` without the head, then `gallery.search(feat8, k)`
        on the same stream (include/ivit_search.h) — the k nearest gallery rows of every image as `predict.search_reference`
        states them.  idx / val are the gallery's buffers for this (B, k), feat8 the engine's: copy=True (or clone) to keep them."""
        feat8 = self.features(images, nslices=nslices)[0]
        idx, val = gallery.search(feat8, k=k)
        out = (idx, val, feat8)
        return tuple(t.clone() for t in out) if copy else out

    def retrieve_within(self, images, gallery, threshold, nslices=1):
        """images int8 [B, C, H, W], gallery an `ivit_amd.search.Gallery` of this backbone's features -> (row_ptr int64 [B + 1], idx
        int32 [total], val float32 [total], feat8 int8 [B, num_features]) device tensors: `features` without the head, then
        `gallery.within(feat8, threshold)` on the same stream (include/ivit_range.h) — every gallery row whose score against an
        image is >= threshold (the cosine for a cosine gallery), by ascending row, as `predict.range_reference` states them.
        `within` synchronises once, to size the result; row_ptr / idx / val are fresh tensors, feat8 the engine's buffer."""
        feat8 = self.features(images, nslices=nslices)[0]
        row_ptr, idx, val = gallery.within(feat8, threshold)
        return row_ptr, idx, val, feat8

    def cluster_assign(self, images, kmeans, nslices=1, copy=False):
        """images int8 [B, C, H, W], kmeans an `ivit_amd.cluster.KMeans` over this backbone's features -> (assign int32 [B], dist2
        int32 [B], feat8 int8 [B, num_features]) device tensors: `features` without the head, then `kmeans.assign(feat8)` on the
        same stream (include/ivit_cluster.h) — every image's nearest centroid and its exact squared distance as
        `predict.kmeans_assign_reference` states them.  assign / dist2 are the KMeans' buffers for this B, feat8 the engine's:
        copy=True (or clone) to keep them."""
        feat8 = self.features(images, nslices=nslices)[0]
        assign, dist2 = kmeans.assign(feat8)
        out = (assign, dist2, feat8)
        return tuple(t.clone() for t in out) if copy else out

    # ---- views (include/ivit_views.h, ivit_amd/views.py): the mean logits of the V views of every image
    def _make_view_buffers(self, G, k):
        ncls = self.cfg.num_classes
        if k:
            return self._empty(torch.int32, G, ncls), self._empty(torch.int32, G, k), self._empty(torch.float32, G, k)
        return self._empty(torch.int32, G, ncls), self._empty(torch.int32, G), self._empty(torch.float64, G)

    def view_scale(self, views):
        """device float32 [num_classes]: fl32(head_scale / fl32(views)), the scale of a sum over `views` views
        (`predict.view_scale_reference`); made once per `views` and kept"""
        if views not in self._view_scale:
            from .predict import view_scale_reference
            self._view_scale[views] = torch.from_numpy(view_scale_reference(self.head_scale_host(), views)).to(self.device)
        return self._view_scale[views]

    @staticmethod
    def _view_groups(images, views):
        """number of images behind a batch of views; ValueError where `views` is outside 1 .. 64 or the batch no multiple of it"""
        from .predict import MAX_VIEWS
        if not isinstance(views, (int, np.integer)) or not 1 <= views <= MAX_VIEWS:
            raise ValueError(f"views = {views!r} outside 1 .. {MAX_VIEWS}")
        if images.shape[0] % views:
            raise ValueError(f"{images.shape[0]} images are no multiple of {views} views")
        return images.shape[0] // int(views)

    def _view_sum(self, images, views, k, nslices):
        """forward on the G * views images, then ivit_logits_view_sum on the same stream -> (G, scale vector, (sum, two side buffers))"""
        G, views = self._view_groups(images, views), int(views)
        scale = self.view_scale(views)                      # before the forward: its upload is made once, not in the loop
        logits = self.forward(images, nslices=nslices)
        bufs = self._views_out.get((G, int(k)))
        self.h.call("ivit_logits_view_sum", _ptr(logits), G, views, self.cfg.num_classes, _ptr(bufs[0]))
        return G, scale, bufs

    def predict_views(self, images, views, k=5, nslices=1, copy=False):
        """images int8 [G * views, C, H, W], the views of an image in consecutive rows (ivit_amd.views.view_transform of an
        image-major table) -> (idx int32 [G, k], val float32 [G, k], logits_sum int32 [G, num_classes]) device tensors: `predict`
        on the MEAN logits of every image's views.  The forward on all G * views images, then ivit_logits_view_sum (the integer
        sum, saturated: `predict.view_sum_reference`) and ivit_logits_topk with the scale vector fl32(head_scale / fl32(views)),
        on the same stream: idx and val are `predict.topk_reference` of the sum with `view_scale(views)`.  ValueError before
        anything runs where views is outside 1 .. 64 or the batch is no multiple of it.  The results are the engine's own buffers
        for this (G, k): copy=True (or clone) to keep them across calls."""
        k = int(k)
        if not 1 <= k <= min(16, self.cfg.num_classes):
            raise ValueError(f"k = {k} outside 1 .. min(16, {self.cfg.num_classes})")
        G, scale, (total, idx, val) = self._view_sum(images, views, k, nslices)
        self.h.call("ivit_logits_topk", _ptr(total), _ptr(scale), G, self.cfg.num_classes, k, _ptr(idx), _ptr(val))
        out = (idx, val, total)
        return tuple(t.clone() for t in out) if copy else out

    def score_views(self, images, labels, views, nslices=1, copy=False):
        """images int8 [G * views, C, H, W] as `predict_views` takes them, labels int64 device tensor [G] -> (rank int32 [G], nll
        float64 [G]): `score` on the MEAN logits of every image's views — `predict.score_reference` of the views' integer sum with
        `view_scale(views)`.  Forward, ivit_logits_view_sum and ivit_logits_score on the same stream."""
        self._check_labels(labels, self._view_groups(images, views))
        G, scale, (total, rank, nll) = self._view_sum(images, views, 0, nslices)
        self.h.call("ivit_logits_score", _ptr(total), _ptr(scale), _ptr(labels), G, self.cfg.num_classes, _ptr(rank), _ptr(nll))
        out = (rank, nll)
        return tuple(t.clone() for t in out) if copy else out

    # ---- linear probe (include/ivit_probe.h, ivit_amd/probe.py): the statistics of a training pass, and the way back into an engine
    def probe_accumulate(self, images, labels, stats, nslices=1):
        """images int8 [B, C, H, W], labels int64 device tensor [B], stats an `ivit_amd.probe.ProbeStats` of this backbone's
        num_features: `features` without the head, then `stats.add(feat8, labels)` on the same stream (ivit_probe_accumulate) — the
        batch's Gram matrix, class sums and counts ADDED into `stats` as `predict.probe_stats_reference` states them; a label outside
        stats.num_classes is ignored.  Nothing is kept of the features and nothing synchronises.  Returns feat8, the engine's own
        buffer for this (batch, nslices)."""
        self._check_labels(labels, images.shape[0])
        feat8 = self.features(images, nslices=nslices)[0]
        stats.add(feat8, labels)
        return feat8

    def _with_head_engine(self, cfg, blob, table, head):
        """a new engine of this class on the repacked constants, through the pre-packed route `load_engine` uses"""
        raise NotImplementedError

    def with_head(self, head):
        """head an `ivit_amd.probe.Head` on this backbone's features -> a NEW engine of the same class with that head in place of
        the one this engine was frozen with: the constants records are taken out of the blob by the table, "head.w", "head.b" and
        "head.scale" replaced, num_classes set (a Swin's class_scale too: fl32(token_scale * weight_scale[c])), repacked with
        `pack_constants`; the input scale and the features' scale are kept.  Every entry of the new engine works on the new classes
        (forward, predict, score, evaluate, class_map, save — and ivit_model_open on the saved file).  This engine is unchanged.
        IvitError where the engine lacks its features' scale, where the head's width is not num_features or where the head was
        quantised on another features' scale."""
        import dataclasses
        from .engine import pack_constants
        s_feat = np.float32(self.feature_scale_host())
        if head.dim != self.num_features:
            raise _lib.IvitError(f"head.weight is [{head.num_classes}, {head.dim}]: this backbone has {self.num_features} features")
        if np.float32(head.feature_scale) != s_feat:
            raise _lib.IvitError(f"the head was quantised on a features' scale of {head.feature_scale!r}, this engine's is {float(s_feat)!r}")
        blob = self.blob.cpu().numpy()
        consts = {}
        for name, (o, dt, shp) in self.table.items():
            n = int(np.prod(shp)) * np.dtype(dt).itemsize
            consts[name] = blob[o:o + n].view(np.dtype(dt)).reshape(shp).copy()
        consts["head.w"] = np.ascontiguousarray(head.w8, np.int8)
        consts["head.b"] = np.ascontiguousarray(head.b32, np.int32)
        consts["head.scale"] = np.ascontiguousarray(head.scale, np.float32)
        blob, table = pack_constants(consts)
        return self._with_head_engine(dataclasses.replace(self.cfg, num_classes=head.num_classes), blob, table, head)

    def _capture(self, suffix, images, args, key, bufs, out, side=None):
        """hipGraph of the entry PREFIX + suffix on fixed buffers; returns a callable that replays it and returns `out`.  `side`:
        the SideOutputs that `key` is then pinned in"""
        if self._gstream is None:
            self._gstream = torch.cuda.Stream(self.device)
        torch.cuda.synchronize(self.device)
        self.h.set_stream(self._gstream.cuda_stream)
        g = _P()
        self._entry(suffix, *args, ctypes.byref(g))
        # the graph replays on its buffers and on `images`: all live as long as the replay closure does, and the workspace
        # entry — with it the side outputs' — is pinned against eviction
        self._graphs.append((g,) + bufs + (images,))
        self._native_ws.pin(key[:2])
        if side is not None:
            side.pin(key)
        lib, gs, dev = self.h.lib, self._gstream, self.device

        def replay(_keep=bufs + (images,)):
            cur = torch.cuda.current_stream(dev)
            gs.wait_stream(cur)
            self.h.set_stream(gs.cuda_stream)
            self.h._check(lib.ivit_graph_launch(g), "ivit_graph_launch")
            cur.wait_stream(gs)
            return out
        return replay

    def capture(self, images, nstreams=1):
        """hipGraph of one forward on fixed buffers (PREFIX_graph_create).  Returns a callable that
        replays it and returns the logits tensor."""
        args, key, bufs = self._args(images, nstreams)
        return self._capture("_graph_create", images, args, key, bufs, bufs[1])

    def capture_predict(self, images, k=5, nstreams=1):
        """hipGraph of one predict on fixed buffers; returns a callable that replays it and returns (idx, val)."""
        self._check_images(images)
        args, key, bufs = self._args(images, nstreams, k)
        return self._capture("_predict_graph_create", images, args, key, bufs, bufs[2:], self._predict_out)

    def capture_score(self, images, labels, nstreams=1):
        """hipGraph of one score on fixed buffers; returns a callable that replays it and returns (rank, nll).  A replay reads
        `images` and `labels` as they are then: both live as long as the callable does."""
        self._check_images(images)
        args, key, bufs = self._score_args(images, labels, nstreams)
        return self._capture("_score_graph_create", images, args, key, bufs + (labels,), bufs[2:4], self._score_out)

    def capture_features(self, images, normalize=False, logits=False, nstreams=1):
        """hipGraph of one features on fixed buffers; returns a callable that replays it and returns what `features` returns."""
        self._check_images(images)
        args, key, bufs = self._features_args(images, normalize, logits, nstreams)
        return self._capture("_features_graph_create", images, args, key, bufs, bufs[2:4] + ((bufs[1],) if logits else ()),
                             self._features_out)

