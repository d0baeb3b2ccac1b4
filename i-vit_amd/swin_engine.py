"""SwinEngine — frozen integer Swin forward on one MI355X through the C-ABI.

Call order of the reference `SwinTransformer.forward_features/forward`
(models/swin_quant.py:539-564; SwinTransformerBlock :251-301; WindowAttention :121-169;
PatchMerging :328-349; PatchEmbed layers_quant.py:184-196) on the fused kernels:

  * activations stay in NATURAL token order [B, R*R, C] for the whole network; torch.roll,
    window_partition and window_reverse exist only as index arithmetic inside
    `ivit_window_attention_fused`;
  * QuantLinear -> QuantAct, IntLayerNorm -> QuantAct, IntGELU -> QuantAct and
    QuantAct -> QuantAct(identity) pairs are single kernels, as in the ViT engine;
  * stage-0 LayerNorms use torch's token-contiguous summation order.

Constants are derived once on the host with the reference's fp32/fp64 operation order
(`freeze.freeze_swin`).  `forward` / `capture` / `predict` / `capture_predict` are NativeEngine's
(ivit_amd.native); `class_map` / `capture_class_map` are this engine's own: the same runner with the
final-stage tokens handed out and the class-activation maps behind them (`ivit_swin_class_map`,
include/ivit_classmap.h); `hidden_states` / `capture_hidden_states` (stage outputs, the feature pyramid,
include/ivit_hidden.h) are NativeEngine's with a Swin's planes; `forward_ops` issues the same forward one C-ABI call per operator.
torch is used for device memory and streams only.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .engine import pack_constants
from .freeze import freeze_swin, quantize_weight         # freeze_swin lives beside freeze_vit; importable from here as before
from .native import NativeEngine, SideOutputs, _ptr

_P = ctypes.c_void_p


DEVICE_DYADICS = ("dy_qact1",)          # [1,2] tables the kernels read through a pointer


def pack_swin_constants(consts):
    """freeze_swin output -> (byte blob, table, host scalars): the unit one RCCL broadcast carries.
    Arrays go into the blob; by-value dyadics and fp32 scalars travel in `host` (a small picklable dict)."""
    arrays, host = {}, {}
    for k, v in consts.items():
        if isinstance(v, np.ndarray) and v.dtype == np.float64 and v.shape == (1, 2) and k not in DEVICE_DYADICS:
            host[k] = ("dy", float(v[0, 0]), float(v[0, 1]))
        elif isinstance(v, np.ndarray) and v.ndim >= 1:
            arrays[k] = v
        else:
            host[k] = ("f", float(np.float32(v)))
    blob, table = pack_constants(arrays)
    return blob, table, host


def packed_swin(cfg, weights, scales, exp_tables=False):
    """pack_swin_constants(freeze_swin(...)), and in its host part the one scale a caller of the engine needs that no constant
    holds: "feat.s", the scale of forward_features' output (qact3, swin_quant.py:555).  What the engine is built from, here and
    behind a broadcast"""
    blob, table, host = pack_swin_constants(freeze_swin(cfg, weights, scales, exp_tables))
    host["feat.s"] = ("f", float(np.float32(scales["qact3"])))
    return blob, table, host


def swin_host_scalars(host):
    """(fp32 scalars, by-value dyadics) from the host part of pack_swin_constants"""
    return ({k: v[1] for k, v in host.items() if v[0] == "f"},
            {k: _lib.Dyadic(v[1], v[2]) for k, v in host.items() if v[0] == "dy"})


def swin_native_params(cfg, table, f, dy, base):
    """(ivit_swin_config, ivit_swin_params, keep-alive) for ivit_swin_create — or its CPU twin: `base` is the address of the
    packed constants blob (device memory for the library, host memory for oracle/ivit_twin.c)"""
    L = _lib
    a = lambda name: (base + table[name][0]) if name in table else None
    ln = lambda p: L.LnParams(a(p + ".bias_int"), a(p + ".sc"), a(p + ".dy"))
    lin = lambda p: L.LinParams(a(p + ".w"), a(p + ".b"), a(p + ".dy"))
    nb = sum(cfg.depths)
    blocks = (L.SwinBlock * nb)()
    merges = (L.SwinMerge * max(1, cfg.num_layers - 1))()
    i = 0
    for li, depth in enumerate(cfg.depths):
        for bj in range(depth):
            p, b = f"layers.{li}.blocks.{bj}.", blocks[i]
            b.s_in, b.n1, b.qkv = f[p + "s_in"], ln(p + "norm1"), lin(p + "attn.qkv")
            b.dy_qk, b.dy_a, b.relb = dy[p + "attn.dy_qk"], dy[p + "attn.dy_a"], a(p + "attn.relb")
            b.s_softmax, b.dy_pv, b.proj = f[p + "attn.s_softmax"], dy[p + "attn.dy_pv"], lin(p + "attn.proj")
            if p + "attn.exp_aq" in table:
                b.exp_aq, b.exp_t, b.exp_cls = a(p + "attn.exp_aq"), a(p + "attn.exp_t"), a(p + "attn.exp_cls")
                b.exp_nc, b.exp_tcount, b.exp_dmin = (int(f[p + "attn.exp_nc"]), int(f[p + "attn.exp_tcount"]),
                                                      int(f[p + "attn.exp_dmin"]))
            b.res1_main, b.res1_res = dy[p + "res1.dy_main"], dy[p + "res1.dy_res"]
            b.s_mid, b.n2, b.fc1 = f[p + "s_mid"], ln(p + "norm2"), lin(p + "mlp.fc1")
            b.s_gelu, b.dy_gelu, b.fc2 = f[p + "mlp.s_gelu"], dy[p + "mlp.dy_gelu"], lin(p + "mlp.fc2")
            b.res2_main, b.res2_res = dy[p + "res2.dy_main"], dy[p + "res2.dy_res"]
            i += 1
        if li < cfg.num_layers - 1:
            p, g = f"layers.{li}.downsample.", merges[li]
            g.s_in, g.n, g.red = f[p + "s_in"], ln(p + "norm"), lin(p + "reduction")
    prm = L.SwinParams()
    prm.pe, prm.s_bn, prm.pn, prm.dy_qact1 = lin("patch_embed.proj"), f["patch_embed.s_bn"], ln("patch_embed.norm"), a("dy_qact1")
    prm.blocks_host = ctypes.addressof(blocks)
    prm.merges_host = ctypes.addressof(merges)
    prm.s_norm_in, prm.n, prm.dy_pool = f["norm.s_in"], ln("norm"), dy["dy_pool"]
    prm.head_w, prm.head_b = a("head.w"), a("head.b")
    prm.s_pool = f["pool.s_in"]
    c = L.SwinConfigC(cfg.img_size, cfg.patch_size, cfg.in_chans, cfg.embed_dim, cfg.num_layers, cfg.window_size,
                      int(cfg.mlp_ratio), cfg.num_classes, (ctypes.c_int * 4)(*(list(cfg.depths) + [0] * 4)[:4]),
                      (ctypes.c_int * 4)(*(list(cfg.num_heads) + [0] * 4)[:4]))
    return c, prm, (blocks, merges)


FUSED_WINDOWS = (7, 12)      # window sizes the fused windowed attention is built for (head dim 32)


def check_swin_windows(cfg):
    """IvitError unless the fused path covers cfg: head dim 32 everywhere, and every stage resolution a multiple of the
    window or at most the window (then the stage is one unshifted window of that resolution, SwinTransformerBlock.__init__),
    with every window that results in FUSED_WINDOWS."""
    if any((cfg.embed_dim * 2 ** i) // h != 32 or (cfg.embed_dim * 2 ** i) % h for i, h in enumerate(cfg.num_heads)):
        raise _lib.IvitError("the fused windowed attention is built for head dim 32")
    for li in range(cfg.num_layers):
        res = cfg.grid // 2 ** li
        wsz = min(cfg.window_size, res)
        if wsz not in FUSED_WINDOWS or res % wsz:
            raise _lib.IvitError(f"the fused windowed attention is built for windows {FUSED_WINDOWS}: stage {li} has "
                                 f"resolution {res} and window {wsz}")


class SwinEngine(NativeEngine):
    PREFIX = "ivit_swin"

    def __init__(self, cfg, weights, scales, device="cuda:0", packed=None, exp_tables=False, input_scale=None, class_scale=None):
        """weights/scales: freeze here (rank 0) — or `packed` = (blob, table, host) received from a broadcast or read from a model
        file.  exp_tables: see freeze_swin.  input_scale, class_scale: what a model file carries beside the package (the scale of
        qact_input; float32 [num_classes], see `class_scale`); by default they come from `scales` and `weights` where those are given."""
        super().__init__(cfg, device)
        if input_scale is None and scales is not None:
            input_scale = scales.get("qact_input")
        self._input_scale = None if input_scale is None else float(np.float32(input_scale))
        check_swin_windows(cfg)
        blob, table, host = packed if packed is not None else packed_swin(cfg, weights, scales, exp_tables)
        self.host_consts = host
        self._load(blob, table)
        self.head_scale = self.head_scale_host()
        self.f, self.dy = swin_host_scalars(host)
        self._build_native()
        # per-layer ShiftGELU(+requant) tables for forward_ops (the native runner owns its own copies)
        self.gelu = {}
        for li, depth in enumerate(cfg.depths):
            for bj in range(depth):
                p = f"layers.{li}.blocks.{bj}."
                tab = torch.empty(65536, dtype=torch.int8, device=self.device)
                self.h.call("ivit_shiftgelu_build_table", self.f[p + "mlp.s_gelu"], self.dy[p + "mlp.dy_gelu"], _P(tab.data_ptr()))
                self.gelu[p] = tab
        self._ws = {}
        # class maps: (idx, val, tok8, cam32, map32) per (batch, slices, k, classes given), beside the logits buffer like every side
        # output; and the unit of a map, fl32(s_tok * fc_scaling_factor[c]) (quant_modules.py:96-97 with qact2's scale in place of
        # qact3's), built here once from the head's float weights: no frozen constant holds the head's weight scale by itself
        self._class_map_out = SideOutputs(self._native_ws)
        self._class_scale = None
        if weights is not None:
            fc_sf = quantize_weight(weights["head.weight"])[1]
            class_scale = (np.float32(self.token_scale_host()) * fc_sf).astype(np.float32)
        if class_scale is not None:
            class_scale = np.ascontiguousarray(class_scale, np.float32)
            assert class_scale.shape == (cfg.num_classes,), "class_scale: float32 [num_classes]"
            self._class_scale = torch.from_numpy(class_scale).to(self.device)
        self._streams = []              # forward_ops with nslices > 1
        self.use_exp_tables = True      # forward_ops only: False issues the arithmetic Shiftmax in every window (cross-check)

    def _native_params(self):
        return swin_native_params(self.cfg, self.table, self.f, self.dy, self.blob.data_ptr())

    def _with_head_engine(self, cfg, blob, table, head):
        class_scale = (np.float32(self.token_scale_host()) * np.asarray(head.weight_scale, np.float32)).astype(np.float32)
        return type(self)(cfg, None, None, device=self.device, packed=(blob, table, dict(self.host_consts)), input_scale=self._input_scale,
                          class_scale=class_scale)

    @property
    def num_features(self):
        return self.cfg.num_features

    def feature_scale_host(self):
        if "feat.s" not in self.f:
            raise _lib.IvitError("this engine was built without the features' scale: build it from weights and scales, or from packed_swin")
        return self.f["feat.s"]

    # ---- class-activation maps and dense token features (include/ivit_classmap.h).  A Swin feature: the final-stage tokens all pass
    # qact2 and so share one scale; ViTEngine has no `class_map` (its patch rows have no scale), SwinEngine still no `attention`
    def token_scale_host(self):
        """host float: the scale of the final-stage tokens' integers (the reference's qact2, swin_quant.py:552)"""
        return self.f["pool.s_in"]

    @property
    def class_scale(self):
        """device float32 [num_classes]: fl32(token_scale * head.fc_scaling_factor[c]), the unit of class c's map"""
        if self._class_scale is None:
            raise _lib.IvitError("this engine was built without the head's float weights (a broadcast package): class_scale needs "
                                 "their per-class scale; build the engine from weights and scales, or load it from a model file")
        return self._class_scale

    def _file_package(self):
        self.feature_scale_host()                   # a file holds "feat.s" and "class_scale": the engine says where either is missing
        return "swin", dict(self.host_consts), {"class_scale": self.class_scale.cpu().numpy()}

    def _class_map_args(self, images, k, classes, logits, nslices):
        """(arguments of the class-map entries, cache key, buffers, what the caller gets) for one batch: val, tok8, cam32, map32 —
        and idx unless the caller gives the classes — live beside the logits buffer and follow its rule (SideOutputs)"""
        cfg, B, C = self.cfg, images.shape[0], self.num_features
        g = cfg.grid >> (cfg.num_layers - 1)
        given = classes is not None
        if given:
            assert isinstance(classes, torch.Tensor) and classes.dtype == torch.int32 and classes.device == self.device, "classes: int32 device tensor"
            assert classes.ndim == 2 and classes.shape[0] == B and classes.is_contiguous(), f"classes must be a contiguous [{B}, k]"
            k = classes.shape[1]
        elif not logits:
            raise ValueError("the k best classes are read off the logits: logits=False goes with classes=")
        k = int(k)
        args, key, (ws, lg) = self._args(images, nslices)
        okey = key + (k, given)
        e = self._empty
        idx, val, tok8, cam32, map32 = self._class_map_out.get(okey, lg, lambda: (
            None if given else e(torch.int32, B, k), None if given else e(torch.float32, B, k), e(torch.int8, B, g * g, C),
            e(torch.int32, B, k, g * g), e(torch.float32, B, k, g * g)))
        if given:
            idx = classes
        mode = _lib.IVIT_CLASSMAP_GIVEN if given else _lib.IVIT_CLASSMAP_TOPK
        args = args[:-1] + (_ptr(lg) if logits else None, self.ptr("head.scale"), mode, k, _ptr(idx), None if given else _ptr(val),
                            _ptr(tok8), _ptr(self.class_scale), _ptr(cam32), _ptr(map32))
        return args, okey, (ws, lg, idx, tok8, cam32, map32) + (() if given else (val,)), (idx, val, tok8, cam32, map32.view(B, k, g, g))

    def class_map(self, images, k=5, classes=None, logits=True, nslices=1, copy=False):
        """images int8 [B, C, H, W] -> (idx, val, tok8, cam32, maps) device tensors: what each final-stage token contributes to a class.
        classes=None: idx int32 [B, k] and val float32 [B, k] are predict's, the k best classes of this forward.  classes = an int32
        device tensor [B, k] (e.g. the labels): those classes — idx is that tensor, val None; an index outside the classes gives a map
        of zeros / NaN.  tok8 int8 [B, L, C]: the tokens behind norm -> qact2 (swin_quant.py:551-552), L = gh * gw in row-major grid
        order, C = num_features, scale `token_scale_host()` — the dense features of the backbone.  cam32 int32 [B, k, L]: the head's
        weight row of the class against every token, exact (`predict.class_map_reference`).  maps float32 [B, k, gh, gw]:
        cam32 * class_scale[class], one multiply.  One native call: the final norm writes the caller's rows, the top-k and ONE launch
        for the maps follow behind the slices' join.  With logits=False (classes given) the forward ends behind the final norm:
        no pool, no head; else the int32 logits are forward's (and `last_logits`).  The results are the engine's own buffers for
        this (batch, nslices, k, mode): copy=True (or clone) to keep them across calls."""
        def plan():
            args, _, bufs, out = self._class_map_args(images, k, classes, logits, nslices)
            return args, bufs[1] if logits else None, out
        out = self._eager("_class_map", images, False, plan)
        return tuple(t if t is None else t.clone() for t in out) if copy else out

    def capture_class_map(self, images, k=5, classes=None, logits=True, nstreams=1):
        """hipGraph of one class_map on fixed buffers; returns a callable that replays it and returns what `class_map` returns.  A
        replay reads `images` — and `classes`, if given — as they are then."""
        self._check_images(images)
        args, okey, bufs, out = self._class_map_args(images, k, classes, logits, nstreams)
        return self._capture("_class_map_graph_create", images, args, okey, bufs, out, self._class_map_out)

    # ---- hidden states (include/ivit_hidden.h): the outputs of chosen stages, NativeEngine's with a Swin's planes
    HIDDEN_SITE = "stage"

    def _hidden_sites(self):
        return self.cfg.num_layers

    def _hidden_plane(self, i):
        res = self.cfg.grid >> i
        return res * res, self.cfg.embed_dim << i, res

    def _hidden_views(self, hid16, hid32, planes, B, layout):
        v16, v32, o16 = [], [], 0
        for L, C, res in planes:                             # no class row: both buffers are packed alike
            v16.append(hid16[o16:o16 + B * L * C].view(B, L, C))
            if hid32 is not None:
                p = hid32[o16:o16 + B * L * C]
                v32.append(p.view(B, C, res, res) if layout == "grid" else p.view(B, L, C))
            o16 += B * L * C
        return tuple(v16), (tuple(v32) if hid32 is not None else None)

    def hidden_states(self, images, stages=-1, layout=None, logits=False, nslices=1, copy=False):
        """images int8 [B, C, H, W] -> (hid16, hid32), or (hid16, hid32, logits) with logits=True: the feature pyramid.  hid16: a
        tuple of int16 views [B, L_s, C_s], one per stage asked for — the output of the stage's last block in front of
        PatchMerging (BasicLayer.forward), L_s = (grid >> s)^2 row-major over the stage's grid, C_s = embed_dim << s, scale
        `hidden_scale_host(s)`.  hid32: None (layout=None) or a tuple of float32 views, [B, L_s, C_s] (layout="tokens") or
        [B, C_s, res_s, res_s] (layout="grid") — `predict.hidden_reference` of the plane.  The views share one packed buffer each.
        See NativeEngine.hidden_states."""
        return super().hidden_states(images, stages, layout, logits, nslices, copy)

    def capture_hidden_states(self, images, stages=-1, layout=None, logits=False, nstreams=1):
        """hipGraph of one hidden_states on fixed buffers; returns a callable that replays it and returns what it returns"""
        return super().capture_hidden_states(images, stages, layout, logits, nstreams)

    def workspace(self, B, key=None):
        if (B, key) in self._ws:
            return self._ws[(B, key)]
        cfg, dev = self.cfg, self.device
        L0, E = cfg.grid * cfg.grid, cfg.embed_dim
        e = lambda n, dt: torch.empty(n, dtype=dt, device=dev)
        M0 = B * L0
        ws = dict(
            patches=e(M0 * cfg.in_chans * cfg.patch_size ** 2, torch.int8),
            a8=e(M0 * E, torch.int8),            # LN output / generic int8 [M, C]
            x16a=e(M0 * E, torch.int16), x16b=e(M0 * E, torch.int16), x16c=e(M0 * E, torch.int16),
            zf=e(M0 * E, torch.float32),
            qkv=e(M0 * 3 * E, torch.int8),
            ctx=e(M0 * E, torch.int8),
            h8=e(M0 * 4 * E, torch.int8), g8=e(M0 * 4 * E, torch.int8),
            pool=e(B * E * 2 ** (cfg.num_layers - 1), torch.int8),
            logits=torch.empty(B, cfg.num_classes, dtype=torch.int32, device=dev),
        )
        self._ws[(B, key)] = ws
        return ws

    def forward_ops(self, images, nslices=1):
        """the same forward issued one C-ABI call per operator from Python (per-operator timing)"""
        if nslices > 1 and images.shape[0] >= nslices:
            return self._forward_sliced(images, nslices)
        return self._forward_one(images, None)

    def _forward_sliced(self, images, nslices):
        B = images.shape[0]
        if len(self._streams) != nslices:
            self._streams = [torch.cuda.Stream(self.device) for _ in range(nslices)]
        cur = torch.cuda.current_stream(self.device)
        bounds = [(B * i) // nslices for i in range(nslices + 1)]
        outs = []
        for i, st in enumerate(self._streams):
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                outs.append(self._forward_one(images[bounds[i]:bounds[i + 1]], ("slice", i)))
        for st in self._streams:
            cur.wait_stream(st)
        return torch.cat(outs, 0)

    def _forward_one(self, images, ws_key):
        cfg, call, f, dy = self.cfg, self.h.call, self.f, self.dy
        assert images.dtype == torch.int8 and images.is_contiguous() and images.device == self.device
        self.h.set_stream(torch.cuda.current_stream(self.device).cuda_stream)
        B = images.shape[0]
        ws = self.workspace(B, ws_key)
        P = lambda t: _P(t.data_ptr())
        E, res = cfg.embed_dim, cfg.grid
        L = res * res
        M = B * L
        Kp = cfg.in_chans * cfg.patch_size ** 2
        # ---- PatchEmbed: conv(4x4/4) -> qact_before_norm(8) -> norm -> qact(16) -> qact1(16)
        call("ivit_im2col_patch", P(images), B, cfg.in_chans, cfg.img_size, cfg.img_size, cfg.patch_size, P(ws["patches"]))
        call("ivit_linear_i8_requant", P(ws["patches"]), self.ptr("patch_embed.proj.w"), self.ptr("patch_embed.proj.b"),
             self.ptr("patch_embed.proj.dy"), 8, P(ws["a8"]), M, E, Kp)
        call("ivit_widen_i8_i16", P(ws["a8"]), P(ws["x16b"]), M * E)
        call("ivit_layernorm_tokenorder", P(ws["x16b"]), M, E, f["patch_embed.s_bn"],
             self.ptr("patch_embed.norm.bias_int"), self.ptr("patch_embed.norm.sc"), L, P(ws["zf"]))
        call("ivit_requant_f32", P(ws["zf"]), self.ptr("patch_embed.norm.dy"), E, None, None, 16, P(ws["x16b"]), M, E)
        call("ivit_requant_i16", P(ws["x16b"]), self.ptr("dy_qact1"), 1, None, None, 16, P(ws["x16a"]), M, E)
        x, y, t16 = ws["x16a"], ws["x16b"], ws["x16c"]
        for li, (depth, heads) in enumerate(zip(cfg.depths, cfg.num_heads)):
            C = E * 2 ** li
            for bj in range(depth):
                p = f"layers.{li}.blocks.{bj}."
                shift = 0 if (bj % 2 == 0 or res <= cfg.window_size) else cfg.window_size // 2
                wsz = min(cfg.window_size, res)
                self._ln(x, M, C, f[p + "s_in"], p + "norm1", L, li == 0, ws["a8"])
                call("ivit_linear_i8_requant", P(ws["a8"]), self.ptr(p + "attn.qkv.w"), self.ptr(p + "attn.qkv.b"),
                     self.ptr(p + "attn.qkv.dy"), 8, P(ws["qkv"]), M, 3 * C, C)
                if p + "attn.exp_aq" in self.table and self.use_exp_tables:
                    call("ivit_window_attention_fused_lut", P(ws["qkv"]), dy[p + "attn.dy_qk"], dy[p + "attn.dy_a"],
                         self.ptr(p + "attn.relb"), f[p + "attn.s_softmax"], self.ptr(p + "attn.exp_aq"),
                         self.ptr(p + "attn.exp_t"), self.ptr(p + "attn.exp_cls"), int(f[p + "attn.exp_nc"]),
                         int(f[p + "attn.exp_tcount"]), int(f[p + "attn.exp_dmin"]), dy[p + "attn.dy_pv"], P(ws["ctx"]),
                         B, res, wsz, shift, heads, C // heads)
                else:
                    call("ivit_window_attention_fused", P(ws["qkv"]), dy[p + "attn.dy_qk"], dy[p + "attn.dy_a"],
                         self.ptr(p + "attn.relb"), f[p + "attn.s_softmax"], dy[p + "attn.dy_pv"], P(ws["ctx"]),
                         B, res, wsz, shift, heads, C // heads)
                call("ivit_linear_i8_requant_residual", P(ws["ctx"]), self.ptr(p + "attn.proj.w"), self.ptr(p + "attn.proj.b"),
                     self.ptr(p + "attn.proj.dy"), dy[p + "res1.dy_main"], dy[p + "res1.dy_res"], P(x), P(y), M, C, C)
                x, y = y, x
                self._ln(x, M, C, f[p + "s_mid"], p + "norm2", L, li == 0, ws["a8"])
                call("ivit_linear_i8_requant", P(ws["a8"]), self.ptr(p + "mlp.fc1.w"), self.ptr(p + "mlp.fc1.b"),
                     self.ptr(p + "mlp.fc1.dy"), 8, P(ws["h8"]), M, 4 * C, C)
                call("ivit_shiftgelu_requant_lut", P(ws["h8"]), M, 4 * C, P(self.gelu[p]), P(ws["g8"]))
                call("ivit_linear_i8_requant_residual", P(ws["g8"]), self.ptr(p + "mlp.fc2.w"), self.ptr(p + "mlp.fc2.b"),
                     self.ptr(p + "mlp.fc2.dy"), dy[p + "res2.dy_main"], dy[p + "res2.dy_res"], P(x), P(y), M, C, 4 * C)
                x, y = y, x
            if li < cfg.num_layers - 1:     # PatchMerging: gather -> LN(4C) -> qact1(8) -> reduction -> qact2(8)
                p = f"layers.{li}.downsample."
                call("ivit_patch_merge_gather", P(x), 16, B, res, C, P(t16))
                res //= 2
                L = res * res
                M = B * L
                self._ln(t16, M, 4 * C, f[p + "s_in"], p + "norm", L, False, ws["a8"])
                call("ivit_linear_i8_requant", P(ws["a8"]), self.ptr(p + "reduction.w"), None,
                     self.ptr(p + "reduction.dy"), 8, P(ws["ctx"]), M, 2 * C, 4 * C)
                call("ivit_widen_i8_i16", P(ws["ctx"]), P(x), M * 2 * C)
        C = E * 2 ** (cfg.num_layers - 1)
        self._ln(x, M, C, f["norm.s_in"], "norm", L, False, ws["a8"])
        call("ivit_avgpool_requant_scaled", P(ws["a8"]), B, L, C, f["pool.s_in"], dy["dy_pool"], P(ws["pool"]))
        call("ivit_linear_i8", P(ws["pool"]), self.ptr("head.w"), self.ptr("head.b"), P(ws["logits"]), B, cfg.num_classes, C)
        return ws["logits"]

    def _ln(self, x16, M, C, s_in, name, L, token_order, out8):
        P = lambda t: _P(t.data_ptr())
        if token_order:
            self.h.call("ivit_layernorm_tokenorder_requant", P(x16), M, C, s_in, self.ptr(name + ".bias_int"),
                        self.ptr(name + ".sc"), self.ptr(name + ".dy"), L, P(out8))
        else:
            self.h.call("ivit_layernorm_requant", P(x16), M, C, C, s_in, self.ptr(name + ".bias_int"),
                        self.ptr(name + ".sc"), self.ptr(name + ".dy"), P(out8))

