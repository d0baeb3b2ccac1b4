"""ViTEngine — frozen integer DeiT/ViT forward on one MI355X through the C-ABI.

`forward` / `capture` / `predict` / `capture_predict` are NativeEngine's (ivit_amd.native): the whole
batch goes to the native runner (`ivit_vit_forward`, csrc/ivit_model.h) in one C call.
`hidden_states` / `capture_hidden_states` (block outputs, include/ivit_hidden.h) are NativeEngine's with a ViT's planes.
`attention` / `capture_attention` are this engine's own: the same runner with the class token's
attention probabilities of chosen blocks tapped (`ivit_vit_attention`, include/ivit_attnmap.h).
`forward_ops` issues the same kernels one C-ABI call at a time from Python (used by the
per-operator timing in bench.py and by the parity tests of the unfused attention path).
Both follow the call order of the reference `VisionTransformer.forward`
(models/vit_quant.py:254-282; Block :130-143; Attention :59-88; Mlp
layers_quant.py:144-153) with the QuantLinear->QuantAct, IntLayerNorm->QuantAct,
IntGELU->QuantAct and QuantAct->QuantAct(identity) pairs fused into single kernels.
torch is used for device memory and streams only.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .freeze import freeze_vit
from .native import NativeEngine, SideOutputs, ascending_indices

_P = ctypes.c_void_p


def _align(n, a=256):
    return (n + a - 1) // a * a


def pack_constants(consts):
    """One contiguous byte blob + table {name: (offset, dtype str, shape)} — the unit
    that is broadcast over RCCL to the other ranks."""
    table, off = {}, 0
    for k in sorted(consts):
        a = np.ascontiguousarray(consts[k])
        table[k] = (off, a.dtype.str, a.shape)
        off = _align(off + a.nbytes)
    blob = np.zeros(off, np.uint8)
    for k, (o, _, _) in table.items():
        a = np.ascontiguousarray(consts[k])
        blob[o:o + a.nbytes] = a.view(np.uint8).reshape(-1)
    return blob, table


def _dy(arr):
    """host [1,2] float64 -> by-value struct ivit_dyadic"""
    return _lib.Dyadic(float(arr[0, 0]), float(arr[0, 1]))


def host_scalars(blob, table):
    """the by-value entries of a packed blob (host numpy): scalar dyadics and the Shiftmax table metadata"""
    host = {}
    for k, (o, dt, shp) in table.items():
        if dt == "<f8" and shp == (1, 2):
            host[k] = blob[o:o + 16].view(np.float64).reshape(1, 2).copy()
        elif k.endswith("exp_meta"):
            host[k] = blob[o:o + 12].view(np.int32).copy()
    return host


def vit_native_params(cfg, table, f32, host, base):
    """(ivit_vit_config, ivit_vit_params, keep-alive) for ivit_vit_create — or for its CPU twin: `base` is the address of
    the packed constants blob, in device memory for the library, in host memory for oracle/ivit_twin.c"""
    L = _lib
    ptr = lambda name: base + table[name][0]
    dy = lambda name: _dy(host[name])
    blocks = (L.VitBlock * cfg.depth)()
    for i in range(cfg.depth):
        p, b = f"blocks.{i}.", blocks[i]
        b.s_ln1, b.n1_bias_int, b.n1_sc, b.n1_dy = f32[p + "ln1.s"], ptr(p + "norm1.bias_int"), ptr(p + "norm1.sc"), ptr(p + "norm1.dy")
        b.qkv_w, b.qkv_b, b.qkv_dy = ptr(p + "attn.qkv.w"), ptr(p + "attn.qkv.b"), ptr(p + "attn.qkv.dy")
        b.dy_qk, b.s_softmax, b.dy_pv = dy(p + "attn.dy_qk"), f32[p + "attn.s_softmax"], dy(p + "attn.dy_pv")
        if p + "attn.exp_meta" in host:        # Shiftmax tables for this layer's scale
            meta = host[p + "attn.exp_meta"]
            b.exp_aq, b.exp_t, b.exp_cls = ptr(p + "attn.exp_aq"), ptr(p + "attn.exp_t"), ptr(p + "attn.exp_cls")
            b.exp_nc, b.exp_tcount, b.exp_dmin = int(meta[0]), int(meta[1]), int(meta[2])
        b.proj_w, b.proj_b, b.proj_dy = ptr(p + "attn.proj.w"), ptr(p + "attn.proj.b"), ptr(p + "attn.proj.dy")
        b.res1_main, b.res1_res = dy(p + "res1.dy_main"), dy(p + "res1.dy_res")
        b.s_ln2, b.n2_bias_int, b.n2_sc, b.n2_dy = f32[p + "ln2.s"], ptr(p + "norm2.bias_int"), ptr(p + "norm2.sc"), ptr(p + "norm2.dy")
        b.fc1_w, b.fc1_b, b.fc1_dy = ptr(p + "mlp.fc1.w"), ptr(p + "mlp.fc1.b"), ptr(p + "mlp.fc1.dy")
        b.s_gelu, b.dy_gelu = f32[p + "mlp.s_gelu"], dy(p + "mlp.dy_gelu")
        b.fc2_w, b.fc2_b, b.fc2_dy = ptr(p + "mlp.fc2.w"), ptr(p + "mlp.fc2.b"), ptr(p + "mlp.fc2.dy")
        b.res2_main, b.res2_res = dy(p + "res2.dy_main"), dy(p + "res2.dy_res")
    prm = L.VitParams()
    prm.pe_w, prm.pe_b, prm.pe_dy = ptr("patch_embed.proj.w"), ptr("patch_embed.proj.b"), ptr("patch_embed.proj.dy")
    prm.z_cls, prm.pos, prm.dy_x, prm.dy_pos = ptr("z_cls"), ptr("pos"), dy("embed.dy_x"), dy("embed.dy_pos")
    prm.blocks_host = ctypes.addressof(blocks)
    prm.s_ln, prm.n_bias_int, prm.n_sc, prm.n_dy = f32["ln.s"], ptr("norm.bias_int"), ptr("norm.sc"), ptr("norm.dy")
    prm.head_w, prm.head_b = ptr("head.w"), ptr("head.b")
    c = L.VitConfig(cfg.img_size, cfg.patch_size, cfg.in_chans, cfg.embed_dim, cfg.depth, cfg.num_heads,
                    cfg.hidden_dim, cfg.num_classes)
    return c, prm, blocks


def frozen_vit(cfg, weights, scales):
    """freeze_vit, and beside its scalars the one scale a caller of the engine needs that no constant holds: "feat.s", the scale of
    forward_features' output (qact2, vit_quant.py:273).  What the engine is built from, here and behind a broadcast"""
    consts, f32 = freeze_vit(cfg, weights, scales)
    return consts, dict(f32, **{"feat.s": np.float32(scales["qact2"])})


class ViTEngine(NativeEngine):
    PREFIX = "ivit_vit"

    def __init__(self, cfg, consts, f32, device="cuda:0", blob=None, table=None, input_scale=None):
        """consts/f32 from freeze.freeze_vit (rank 0) — or a pre-packed (blob, table)
        received from a broadcast or read from a model file (then `consts` may be None).  input_scale: the scale of qact_input;
        by default freeze_vit's "s_in" where f32 holds it."""
        self._plans, self._mlp_plans = {}, {}       # before anything can raise: __del__ reads them
        super().__init__(cfg, device)
        if input_scale is None and "s_in" in f32:
            input_scale = f32["s_in"]
        self._input_scale = None if input_scale is None else float(np.float32(input_scale))
        if blob is None:
            blob, table = pack_constants(consts)
        self.f32 = {k: float(np.float32(v)) for k, v in f32.items()}
        self._load(blob, table)
        # scalar dyadics are passed by value: keep host copies
        self.host = host_scalars(blob if isinstance(blob, np.ndarray) else self.blob.cpu().numpy(), table)
        self._ws = {}
        self._attention_out = SideOutputs(self._native_ws)
        self.fused_attention = (cfg.head_dim == 64 and cfg.num_tokens <= 640)
        self.use_exp_tables = True      # forward_ops only: False issues the arithmetic Shiftmax (cross-check)
        # per-layer ShiftGELU(+requant) tables, built on-device by the faithful kernel code
        self.gelu_tab = torch.empty(cfg.depth, 65536, dtype=torch.int8, device=self.device)
        for i in range(cfg.depth):
            p = f"blocks.{i}."
            self.h.call("ivit_shiftgelu_build_table", self.f32[p + "mlp.s_gelu"], _dy(self.host[p + "mlp.dy_gelu"]),
                        _P(self.gelu_tab[i].data_ptr()))

        # Shiftmax row tables (one gather per score, ivit_attention_fused_rowlut) for the layers whose table lines fit 64 entries
        # and whose requant multipliers are in the kernel's fast range — the per-operator path makes the runner's choice
        self.use_row_tables = True
        self.v_row_major = True         # forward_ops: v row-major into the row-table attention (False: v^T as before)
        self.fuse_ln_qkv = True         # forward_ops: norm1 in the qkv GEMM's prologue where the plan is prepared (False: two launches)
        self.fuse_ln_mlp = True         # forward_ops: norm2 in the head of the fused Mlp's launch (False: two launches)
        # forward_ops: norm2 in the lock-step fused Mlp's activation tiles (ivit_layernorm_mlp_lockstep_planned), tried where the launch above
        # refuses.  Off by default: bench.py's --full accounting prices LayerNorm launches from the two LayerNorm-headed names it knows
        self.fuse_ln_mlp_lockstep = False
        self.fuse_patch_embed = True    # forward_ops: ivit_patch_embed (False: im2col, GEMM, embed_finish)
        self._qkv_prepared = set()
        self.rowtab = {}
        if self.fused_attention:
            for i in range(cfg.depth):
                p = f"blocks.{i}."
                if p + "attn.exp_meta" not in self.host:
                    continue
                meta = self.host[p + "attn.exp_meta"]
                dqk, dpv = self.host[p + "attn.dy_qk"], self.host[p + "attn.dy_pv"]
                if 1 - int(meta[2]) <= 64 and abs(dqk[0, 0] * dqk[0, 1]) < 512.0 and abs(dpv[0, 0] * dpv[0, 1]) < 512.0:
                    t = torch.empty(256, 64, dtype=torch.float32, device=self.device)
                    self.h.call("ivit_shiftmax_rowtable", self.ptr(p + "attn.exp_aq"), self.ptr(p + "attn.exp_t"), self.ptr(p + "attn.exp_cls"),
                                int(meta[0]), int(meta[1]), int(meta[2]), _P(t.data_ptr()))
                    self.rowtab[i] = t

        # frozen-QuantLinear plans of the per-operator path (forward_ops / plan()): built on first use by build_op_plans()
        # — plan creation allocates and synchronises, so callers that time or capture forward_ops call it beforehand; the
        # native runner (forward) holds its own plans, and an engine that only runs forward() no longer keeps a second
        # copy of the fragment-ordered Mlp weights (14 MB for DeiT-S).  use_plans = False issues the unplanned kernels
        self.use_plans = True
        self.use_fused_mlp = True       # forward_ops: ivit_mlp_fused_planned where a fused plan exists (D = 384 or 192)
        self._build_native()

    def build_op_plans(self):
        """ivit_linear_plan_create / ivit_mlp_plan_create for every block (idempotent)."""
        if self._plans:
            return
        cfg = self.cfg
        D, Hd = cfg.embed_dim, cfg.hidden_dim
        for i in range(cfg.depth):
            p = f"blocks.{i}."
            for name, N, K in ((p + "attn.qkv", 3 * D, D), (p + "attn.proj", D, D), (p + "mlp.fc1", Hd, D), (p + "mlp.fc2", D, Hd)):
                self._plans[name] = self.h.linear_plan(self.ptr(name + ".w"), self.ptr(name + ".b"), self.ptr(name + ".dy"), N, K)
                if name.endswith("attn.qkv") and D == 384 and D // cfg.num_heads == 64 and \
                        self.h.lib.ivit_linear_plan_prepare_ws(self.h.h, self._plans[name].p) == 0:
                    self._qkv_prepared.add(name)       # gemm_ws_qkv_kernel's weight order: ldv = 0 calls and the fused norm1 form use it
                if name.endswith("attn.proj") and D == 384:     # ... and attn.proj + the residual QuantAct (the runner's choice)
                    self.h.lib.ivit_linear_plan_prepare_ws(self.h.h, self._plans[name].p)
            mp = _P()
            if self.h.lib.ivit_mlp_plan_create(self.h.h, self._plans[p + "mlp.fc1"].p, self._plans[p + "mlp.fc2"].p, ctypes.byref(mp)) == 0:
                self._mlp_plans[i] = mp

    def plan(self, prefix):
        """frozen-QuantLinear plan (ivit_linear_plan_create) of the layer `prefix`; the native runner holds its own."""
        self.build_op_plans()
        return self._plans[prefix].p

    def _native_params(self):
        return vit_native_params(self.cfg, self.table, self.f32, self.host, self.blob.data_ptr())

    def _workspace_init(self, ws, B, nslices):
        self._entry("_workspace_init", self.model, _P(ws.data_ptr()), ws.numel(), B, nslices)

    def __del__(self):
        super().__del__()
        try:
            for mp in self._mlp_plans.values():
                self.h.lib.ivit_mlp_plan_destroy(mp)
            self._mlp_plans = {}
            for pl in self._plans.values():
                pl.close()
        except Exception:
            pass

    @classmethod
    def from_float(cls, cfg, weights, scales, device="cuda:0"):
        consts, f32 = frozen_vit(cfg, weights, scales)
        return cls(cfg, consts, f32, device)

    def head_scale(self):
        return self.head_scale_host()

    def _file_package(self):
        self.feature_scale_host()                   # a file holds "feat.s": the engine says what to do where it is missing
        return "vit", {k: ("f", v) for k, v in self.f32.items()}, {}

    def _with_head_engine(self, cfg, blob, table, head):
        return type(self)(cfg, None, dict(self.f32), device=self.device, blob=blob, table=table, input_scale=self._input_scale)

    @property
    def num_features(self):
        return self.cfg.embed_dim

    def feature_scale_host(self):
        if "feat.s" not in self.f32:
            raise _lib.IvitError("this engine was built without the features' scale: build it with ViTEngine.from_float or frozen_vit")
        return self.f32["feat.s"]

    # ---- the class token's attention rows (include/ivit_attnmap.h).  A ViT / DeiT feature: SwinEngine has no `attention`, a Swin has
    # no class token
    def _attention_blocks(self, blocks):
        """an int or a sequence of block indices, negative ones counting from the end -> strictly ascending tuple in [0, depth)"""
        return ascending_indices(blocks, self.cfg.depth, "block")

    def _attention_args(self, images, blocks, heads, logits, nslices):
        """(arguments of the attention entries, cache key, buffers, what the caller gets) for one batch: attn16 and map32 live beside the
        logits buffer and follow its rule (native.SideOutputs), one set per (batch, slices, blocks, heads)"""
        blocks = self._attention_blocks(blocks)
        args, key, (ws, lg) = self._args(images, nslices)
        cfg, n, B = self.cfg, len(blocks), images.shape[0]
        H, T, g = cfg.num_heads, cfg.num_tokens, cfg.img_size // cfg.patch_size
        assert T == g * g + 1, "one class token in front of a square grid of patches"
        okey = key + (blocks, bool(heads))
        attn16, map32, blocks_host = self._attention_out.get(okey, lg, lambda: (
            self._empty(torch.uint16, n, B, H, T), self._empty(torch.float32, *((n, B, H, T - 1) if heads else (n, B, T - 1))),
            (ctypes.c_int * n)(*blocks)))
        mode = _lib.IVIT_ATTNMAP_HEADS if heads else _lib.IVIT_ATTNMAP_MEAN
        args = args[:-1] + (_P(lg.data_ptr()) if logits else None, blocks_host, n, _P(attn16.data_ptr()), mode, _P(map32.data_ptr()))
        maps = map32.view(n, B, H, g, g) if heads else map32.view(n, B, g, g)
        return args, okey, (ws, lg, attn16, map32, blocks_host), (attn16, maps) + ((lg,) if logits else ())

    def attention(self, images, blocks=-1, heads=False, logits=False, nslices=1, copy=False):
        """images int8 [B, C, H, W] -> (attn16, maps), or (attn16, maps, logits) with logits=True: what the class token attends to in
        the blocks asked for (an int or a sequence; negative indices count from the end; strictly ascending after that, else
        ValueError).  attn16 uint16 [n, B, heads, T]: plane t is row 0 of blocks.{blocks[t]}.attn.int_softmax of the reference
        (vit_quant.py:76), the same integers, scale 2^-15 (`predict.attention_reference`).  maps float32 [n, B, gh, gw]: the
        patch columns of those rows on the patch grid, the mean over the heads — or [n, B, heads, gh, gw] with heads=True, each
        head's own (`predict.attention_map_reference`).  One native call: one small launch per tapped block behind its qkv launch
        and one for the maps.  Without `logits` the forward ends behind the last tapped block; with it the int32 logits are
        forward's (and `last_logits`).  The results are the engine's own buffers for this (batch, nslices, blocks, heads):
        copy=True (or clone) to keep them across calls."""
        def plan():
            args, _, bufs, out = self._attention_args(images, blocks, heads, logits, nslices)
            return args, bufs[1] if logits else None, out
        return self._eager("_attention", images, copy, plan)

    def capture_attention(self, images, blocks=-1, heads=False, logits=False, nstreams=1):
        """hipGraph of one attention on fixed buffers; returns a callable that replays it and returns what `attention` returns."""
        self._check_images(images)
        args, okey, bufs, out = self._attention_args(images, blocks, heads, logits, nstreams)
        return self._capture("_attention_graph_create", images, args, okey, bufs, out, self._attention_out)

    # ---- hidden states (include/ivit_hidden.h): the outputs of chosen blocks, NativeEngine's with a ViT's planes
    HIDDEN_CLASS_ROW = True
    HIDDEN_SITE = "block"

    def _hidden_sites(self):
        return self.cfg.depth

    def _hidden_plane(self, i):
        return self.cfg.num_tokens, self.cfg.embed_dim, self.cfg.img_size // self.cfg.patch_size

    def _hidden_views(self, hid16, hid32, planes, B, layout):
        (T, D, g), n = planes[0], len(planes)
        assert T == g * g + 1, "one class token in front of a square grid of patches"
        if hid32 is not None:
            hid32 = hid32.view(n, B, D, g, g) if layout == "grid" else hid32.view(n, B, T, D)
        return hid16.view(n, B, T, D), hid32

    def hidden_states(self, images, blocks=-1, layout=None, logits=False, nslices=1, copy=False):
        """images int8 [B, C, H, W] -> (hid16, hid32), or (hid16, hid32, logits) with logits=True: the outputs of the blocks asked
        for (normalised as `attention`'s are).  hid16 int16 [n, B, T, D]: plane j holds the integers of
        blocks.{blocks[j]}.qact4 of the reference (vit_quant.py:141-143), class row included, scale `hidden_scale_host(blocks[j])`.
        hid32: None (layout=None), float32 [n, B, T, D] (layout="tokens") or [n, B, D, gh, gw] (layout="grid": the patch rows on
        the patch grid, channel-major; the class token has no place there) — `predict.hidden_reference` of hid16.  See
        NativeEngine.hidden_states; a tap of the last block runs that block on all rows, the logits are forward's all the same."""
        return super().hidden_states(images, blocks, layout, logits, nslices, copy)

    def capture_hidden_states(self, images, blocks=-1, layout=None, logits=False, nstreams=1):
        """hipGraph of one hidden_states on fixed buffers; returns a callable that replays it and returns what it returns"""
        return super().capture_hidden_states(images, blocks, layout, logits, nstreams)

    def workspace(self, B, key=None):
        wkey = (B, key)
        if wkey in self._ws:
            return self._ws[wkey]
        cfg, dev = self.cfg, self.device
        T, D, H, dh, Hd = cfg.num_tokens, cfg.embed_dim, cfg.num_heads, cfg.head_dim, cfg.hidden_dim
        ld = (T + 15) // 16 * 16
        M = B * T
        Kp = cfg.in_chans * cfg.patch_size ** 2
        e = lambda *s, dt: torch.empty(s, dtype=dt, device=dev)
        ws = dict(
            ld=ld,
            patches=e(B * cfg.num_patches, Kp, dt=torch.int8),
            patch16=e(B * cfg.num_patches, D, dt=torch.int16),
            xa=e(M, D, dt=torch.int16), xb=e(M, D, dt=torch.int16),
            a8=e(M, D, dt=torch.int8),
            q=e(B * H, T, dh, dt=torch.int8), k=e(B * H, T, dh, dt=torch.int8),
            vt=torch.zeros(B * H, dh, ld, dtype=torch.int8, device=dev),
            s8=e(B * H, T, ld, dt=torch.int8),
            p16=torch.zeros(B * H, T, ld, dtype=torch.int16, device=dev),  # uint16 payload
            ctx8=e(M, D, dt=torch.int8),
            h8=e(M, Hd, dt=torch.int8), g8=e(M, Hd, dt=torch.int8),
            cls8=e(B, D, dt=torch.int8),
            logits=e(B, cfg.num_classes, dt=torch.int32),
        )
        self._ws[wkey] = ws
        return ws

    def forward_ops(self, images, ws_key=None):
        """The same forward issued one C-ABI call per operator from Python (per-operator timing,
        unfused-attention parity).  Returns int32 logits [B, num_classes]."""
        cfg, call, f32, hc = self.cfg, self.h.call, self.f32, self.host
        assert images.dtype == torch.int8 and images.is_contiguous() and images.device == self.device
        self.h.set_stream(torch.cuda.current_stream(self.device).cuda_stream)
        if self.use_plans:
            self.build_op_plans()
        B = images.shape[0]
        T, D, H, dh, Hd = cfg.num_tokens, cfg.embed_dim, cfg.num_heads, cfg.head_dim, cfg.hidden_dim
        M = B * T
        ws = self.workspace(B, ws_key)
        ld = ws["ld"]
        P = lambda t: _P(t.data_ptr())
        Kp = cfg.in_chans * cfg.patch_size ** 2
        x, y = ws["xa"], ws["xb"]
        # the runner's choice: the whole PatchEmbed front end as one GEMM launch where it applies (16 x 16 patches, fast multipliers)
        one = self.fuse_patch_embed and self.h.try_call(
            "ivit_patch_embed", P(images), B, cfg.in_chans, cfg.img_size, cfg.img_size, cfg.patch_size, self.ptr("patch_embed.proj.w"),
            self.ptr("patch_embed.proj.b"), self.ptr("patch_embed.proj.dy"), self.ptr("z_cls"), self.ptr("pos"), _dy(hc["embed.dy_x"]),
            _dy(hc["embed.dy_pos"]), P(x), D)
        if not one:
            call("ivit_im2col_patch", P(images), B, cfg.in_chans, cfg.img_size, cfg.img_size, cfg.patch_size,
                 P(ws["patches"]))
            call("ivit_linear_i8_requant", P(ws["patches"]), self.ptr("patch_embed.proj.w"),
                 self.ptr("patch_embed.proj.b"), self.ptr("patch_embed.proj.dy"), 16, P(ws["patch16"]),
                 B * cfg.num_patches, D, Kp)
            call("ivit_embed_finish", P(ws["patch16"]), self.ptr("z_cls"), self.ptr("pos"), _dy(hc["embed.dy_x"]),
                 _dy(hc["embed.dy_pos"]), P(x), B, T, D)
        for i in range(cfg.depth):
            p = f"blocks.{i}."
            # the runner's choice (csrc/ivit_model.h): v ROW-major (ldv = 0) between the planned qkv GEMM and the row-table attention
            row_attn = self.fused_attention and i in self.rowtab and self.use_exp_tables and self.use_row_tables
            ldv = 0 if (row_attn and self.use_plans and self.v_row_major) else ld
            # ... and norm1 inside that GEMM's prologue where its plan is prepared (D = 384, dh = 64: ivit_layernorm_linear_i8_qkv_planned)
            fused_ln = ldv == 0 and self.fuse_ln_qkv and (p + "attn.qkv") in self._qkv_prepared
            if not fused_ln:
                call("ivit_layernorm_requant", P(x), M, D, D, f32[p + "ln1.s"], self.ptr(p + "norm1.bias_int"),
                     self.ptr(p + "norm1.sc"), self.ptr(p + "norm1.dy"), P(ws["a8"]))
            if fused_ln:
                call("ivit_layernorm_linear_i8_qkv_planned", self.plan(p + "attn.qkv"), P(x), f32[p + "ln1.s"], self.ptr(p + "norm1.bias_int"),
                     self.ptr(p + "norm1.sc"), self.ptr(p + "norm1.dy"), P(ws["q"]), P(ws["k"]), P(ws["vt"]), B, T, H, dh)
            elif self.use_plans:
                call("ivit_linear_i8_qkv_planned", self.plan(p + "attn.qkv"), P(ws["a8"]), P(ws["q"]), P(ws["k"]),
                     P(ws["vt"]), B, T, H, dh, ldv)
            else:
                call("ivit_linear_i8_qkv", P(ws["a8"]), self.ptr(p + "attn.qkv.w"), self.ptr(p + "attn.qkv.b"),
                     self.ptr(p + "attn.qkv.dy"), P(ws["q"]), P(ws["k"]), P(ws["vt"]), B, T, H, dh, ld)
            if self.fused_attention:
                if row_attn:
                    call("ivit_attention_fused_rowlut", P(ws["q"]), P(ws["k"]), P(ws["vt"]), _dy(hc[p + "attn.dy_qk"]),
                         f32[p + "attn.s_softmax"], P(self.rowtab[i]), int(hc[p + "attn.exp_meta"][2]),
                         _dy(hc[p + "attn.dy_pv"]), P(ws["ctx8"]), B, H, T, dh, ldv)
                elif p + "attn.exp_meta" in hc and self.use_exp_tables:
                    meta = hc[p + "attn.exp_meta"]
                    call("ivit_attention_fused_lut", P(ws["q"]), P(ws["k"]), P(ws["vt"]), _dy(hc[p + "attn.dy_qk"]),
                         f32[p + "attn.s_softmax"], self.ptr(p + "attn.exp_aq"), self.ptr(p + "attn.exp_t"),
                         self.ptr(p + "attn.exp_cls"), int(meta[0]), int(meta[1]), int(meta[2]),
                         _dy(hc[p + "attn.dy_pv"]), P(ws["ctx8"]), B, H, T, dh, ld)
                else:
                    call("ivit_attention_fused", P(ws["q"]), P(ws["k"]), P(ws["vt"]), _dy(hc[p + "attn.dy_qk"]),
                         f32[p + "attn.s_softmax"], _dy(hc[p + "attn.dy_pv"]), P(ws["ctx8"]), B, H, T, dh, ld)
            else:
                call("ivit_attn_qk_requant", P(ws["q"]), P(ws["k"]), _dy(hc[p + "attn.dy_qk"]), P(ws["s8"]),
                     B * H, T, dh, ld)
                call("ivit_shiftmax", P(ws["s8"]), B * H * T, T, ld, f32[p + "attn.s_softmax"], 16, P(ws["p16"]), ld)
                call("ivit_attn_pv_requant", P(ws["p16"]), P(ws["vt"]), _dy(hc[p + "attn.dy_pv"]), P(ws["ctx8"]),
                     B, H, T, dh, ld, ld)
            if self.use_plans:
                call("ivit_linear_i8_requant_residual_planned", self.plan(p + "attn.proj"), P(ws["ctx8"]),
                     _dy(hc[p + "res1.dy_main"]), _dy(hc[p + "res1.dy_res"]), P(x), P(y), M)
            else:
                call("ivit_linear_i8_requant_residual", P(ws["ctx8"]), self.ptr(p + "attn.proj.w"), self.ptr(p + "attn.proj.b"),
                     self.ptr(p + "attn.proj.dy"), _dy(hc[p + "res1.dy_main"]), _dy(hc[p + "res1.dy_res"]), P(x), P(y), M, D, D)
            x, y = y, x
            dm, dr = hc[p + "res2.dy_main"], hc[p + "res2.dy_res"]
            fused = (self.use_plans and self.use_fused_mlp and i in self._mlp_plans
                     and abs(dm[0, 0] * dm[0, 1]) < 512.0 and abs(dr[0, 0] * dr[0, 1]) < 512.0)
            # the runner's choice: norm2 in the head of the fused Mlp's launch where that launch runs on the role-split kernel
            ln_mlp = fused and self.fuse_ln_mlp and self.h.try_call(
                "ivit_layernorm_mlp_fused_planned", self._mlp_plans[i], P(x), f32[p + "ln2.s"], self.ptr(p + "norm2.bias_int"), self.ptr(p + "norm2.sc"),
                self.ptr(p + "norm2.dy"), P(ws["a8"]), _P(self.gelu_tab[i].data_ptr()), _dy(dm), _dy(dr), P(y), M)
            ln_mlp = ln_mlp or (fused and self.fuse_ln_mlp_lockstep and self.h.try_call(
                "ivit_layernorm_mlp_lockstep_planned", self._mlp_plans[i], P(x), f32[p + "ln2.s"], self.ptr(p + "norm2.bias_int"), self.ptr(p + "norm2.sc"),
                self.ptr(p + "norm2.dy"), _P(self.gelu_tab[i].data_ptr()), _dy(dm), _dy(dr), P(y), M))
            if not ln_mlp:
                call("ivit_layernorm_requant", P(x), M, D, D, f32[p + "ln2.s"], self.ptr(p + "norm2.bias_int"),
                     self.ptr(p + "norm2.sc"), self.ptr(p + "norm2.dy"), P(ws["a8"]))
            if ln_mlp:
                pass
            elif fused:       # hidden tensor never in HBM
                call("ivit_mlp_fused_planned", self._mlp_plans[i], P(ws["a8"]), _P(self.gelu_tab[i].data_ptr()), _dy(dm), _dy(dr),
                     P(x), P(y), M)
            elif self.use_plans:
                call("ivit_linear_i8_requant_planned", self.plan(p + "mlp.fc1"), P(ws["a8"]), 8, P(ws["h8"]), M)
                call("ivit_shiftgelu_requant_lut", P(ws["h8"]), M, Hd, _P(self.gelu_tab[i].data_ptr()), P(ws["g8"]))
                call("ivit_linear_i8_requant_residual_planned", self.plan(p + "mlp.fc2"), P(ws["g8"]), _dy(dm), _dy(dr), P(x), P(y), M)
            else:
                call("ivit_linear_i8_requant", P(ws["a8"]), self.ptr(p + "mlp.fc1.w"), self.ptr(p + "mlp.fc1.b"),
                     self.ptr(p + "mlp.fc1.dy"), 8, P(ws["h8"]), M, Hd, D)
                call("ivit_shiftgelu_requant_lut", P(ws["h8"]), M, Hd, _P(self.gelu_tab[i].data_ptr()), P(ws["g8"]))
                call("ivit_linear_i8_requant_residual", P(ws["g8"]), self.ptr(p + "mlp.fc2.w"), self.ptr(p + "mlp.fc2.b"),
                     self.ptr(p + "mlp.fc2.dy"), _dy(dm), _dy(dr), P(x), P(y), M, D, Hd)
            x, y = y, x
        # final norm on the class-token rows only (row stride T*D)
        call("ivit_layernorm_requant", P(x), B, D, T * D, f32["ln.s"], self.ptr("norm.bias_int"),
             self.ptr("norm.sc"), self.ptr("norm.dy"), P(ws["cls8"]))
        call("ivit_linear_i8", P(ws["cls8"]), self.ptr("head.w"), self.ptr("head.b"), P(ws["logits"]),
             B, cfg.num_classes, D)
        self.last_x = x
        return ws["logits"]
