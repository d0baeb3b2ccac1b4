"""ctypes binding of the C-ABI in include/ivit.h (libivit_hip.so, built in-tree).

The product path has NO CPU fallback: if the HIP library is missing or a call
fails, an exception is raised.
"""
import ctypes
import os
import subprocess

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
SO_PATH = os.environ.get("IVIT_LIB") or os.path.join(_CSRC, "libivit_hip.so")
# the one translation unit and every header it may include: an edit to any of them rebuilds the library
SOURCES = ["ivit_hip.hip"] + sorted(f for f in os.listdir(_CSRC) if f.endswith(".h"))
_THIS = os.path.abspath(__file__)
# -packed-fp32-ops: no v_pk_{add,mul,fma}_f32 anywhere in the library.  Round 4 traced the sporadic one-LSB differences of
# layernorm_reg_kernel<192, 1> beside QuantLinear GEMM workgroups to that instruction class; round 5 to one form of it:
# v_pk_{add,mul}_f32 with op_sel:[0,1] reads src1's high dword as 0 on lanes 48..63 while another wave of the SIMD has MFMAs in
# flight (profiles/r05_hazard/README.md, tools/ubench/pk_opsel_hazard.hip).  The flag costs < 1 % (DeiT-B) and
# tests/test_cabi_cpu.py::test_no_packed_fp32_in_library keeps it in place.
# Scoping (the unscoped -Xclang pair also reaches the x86 host compile, which prints "not a recognized feature ...
# ignoring" per function): -Xarch_device refuses to forward cc1 options ("options requiring arguments are unsupported"), and the
# source-level form — target("no-packed-fp32-ops") on every function of the device pass by #pragma clang attribute — produces
# the same 0 v_pk instructions but a 35 % slower DeiT-S forward (4.61 vs 3.02 ms on one box: differing target features keep the
# inliner away from the __forceinline__ helpers), so the command-line form stays; the host-side warning is harmless and the ISA
# test fails if a toolchain ever turns it into a dropped flag.
# gfx950 only, SRAM-ECC on (the only mode MI355X ships in): ivit_mlp_rs.h / ivit_swin_mlp_rs.h rely on ds_read_u8_d16_hi ZEROING the low
# half of its destination, which is the d16 behaviour of SRAM-ECC parts; a target without it would need the merge written out.
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-pass-failed", "-fPIC", "-shared",
               "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]


IVIT_OK, IVIT_ERR_INVALID, IVIT_ERR_HIP, IVIT_ERR_UNSUPPORTED, IVIT_ERR_NO_DEVICE = 0, 1, 2, 3, 4      # include/ivit.h


class IvitError(RuntimeError):
    pass


class Dyadic(ctypes.Structure):
    """struct ivit_dyadic {double m; double r;}"""
    _fields_ = [("m", ctypes.c_double), ("r", ctypes.c_double)]


def build(force=False, verbose=False):
    """Compile the HIP extension for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(_CSRC, s) for s in SOURCES]
    hdr = os.path.join(os.path.dirname(_CSRC), "..", "include", "ivit.h")
    newest = max(os.path.getmtime(p) for p in srcs + [hdr, _THIS])      # the flags live in this file
    if not force and os.path.exists(SO_PATH) and os.path.getmtime(SO_PATH) >= newest:
        return SO_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # one builder at a time (the ranks of a multi-GPU launch import this module together), and the library appears atomically:
    # a rank that lost the race finds it up to date once it holds the lock
    import fcntl
    with open(SO_PATH + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and os.path.exists(SO_PATH) and os.path.getmtime(SO_PATH) >= newest:
            return SO_PATH
        tmp = "%s.%d.tmp" % (SO_PATH, os.getpid())
        cmd = [hipcc] + HIPCC_FLAGS + [os.path.join(_CSRC, "ivit_hip.hip"), "-o", tmp]
        if verbose:
            print(" ".join(cmd))
        try:
            subprocess.check_call(cmd)
            os.replace(tmp, SO_PATH)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
    return SO_PATH


class VitConfig(ctypes.Structure):
    """struct ivit_vit_config"""
    _fields_ = [(n, ctypes.c_int) for n in ("img_size", "patch_size", "in_chans", "embed_dim", "depth", "num_heads",
                                             "hidden_dim", "num_classes")]


class VitBlock(ctypes.Structure):
    """struct ivit_vit_block (device pointers + host scalars of one transformer block)"""
    _fields_ = [
        ("s_ln1", ctypes.c_float), ("n1_bias_int", ctypes.c_void_p), ("n1_sc", ctypes.c_void_p), ("n1_dy", ctypes.c_void_p),
        ("qkv_w", ctypes.c_void_p), ("qkv_b", ctypes.c_void_p), ("qkv_dy", ctypes.c_void_p),
        ("dy_qk", Dyadic), ("s_softmax", ctypes.c_float), ("dy_pv", Dyadic),
        ("exp_aq", ctypes.c_void_p), ("exp_t", ctypes.c_void_p), ("exp_cls", ctypes.c_void_p),
        ("exp_nc", ctypes.c_int), ("exp_tcount", ctypes.c_int), ("exp_dmin", ctypes.c_int),
        ("proj_w", ctypes.c_void_p), ("proj_b", ctypes.c_void_p), ("proj_dy", ctypes.c_void_p),
        ("res1_main", Dyadic), ("res1_res", Dyadic),
        ("s_ln2", ctypes.c_float), ("n2_bias_int", ctypes.c_void_p), ("n2_sc", ctypes.c_void_p), ("n2_dy", ctypes.c_void_p),
        ("fc1_w", ctypes.c_void_p), ("fc1_b", ctypes.c_void_p), ("fc1_dy", ctypes.c_void_p),
        ("s_gelu", ctypes.c_float), ("dy_gelu", Dyadic),
        ("fc2_w", ctypes.c_void_p), ("fc2_b", ctypes.c_void_p), ("fc2_dy", ctypes.c_void_p),
        ("res2_main", Dyadic), ("res2_res", Dyadic),
    ]


class VitParams(ctypes.Structure):
    """struct ivit_vit_params"""
    _fields_ = [
        ("pe_w", ctypes.c_void_p), ("pe_b", ctypes.c_void_p), ("pe_dy", ctypes.c_void_p),
        ("z_cls", ctypes.c_void_p), ("pos", ctypes.c_void_p), ("dy_x", Dyadic), ("dy_pos", Dyadic),
        ("blocks_host", ctypes.POINTER(VitBlock)),
        ("s_ln", ctypes.c_float), ("n_bias_int", ctypes.c_void_p), ("n_sc", ctypes.c_void_p), ("n_dy", ctypes.c_void_p),
        ("head_w", ctypes.c_void_p), ("head_b", ctypes.c_void_p),
    ]


class LnParams(ctypes.Structure):
    """struct ivit_ln_params"""
    _fields_ = [("bias_int", ctypes.c_void_p), ("sc", ctypes.c_void_p), ("dy", ctypes.c_void_p)]


class LinParams(ctypes.Structure):
    """struct ivit_lin_params"""
    _fields_ = [("w", ctypes.c_void_p), ("b", ctypes.c_void_p), ("dy", ctypes.c_void_p)]


class SwinConfigC(ctypes.Structure):
    """struct ivit_swin_config"""
    _fields_ = [(n, ctypes.c_int) for n in ("img_size", "patch_size", "in_chans", "embed_dim", "num_layers", "window_size",
                                             "mlp_ratio", "num_classes")] + [("depths", ctypes.c_int * 4), ("num_heads", ctypes.c_int * 4)]


class SwinBlock(ctypes.Structure):
    """struct ivit_swin_block"""
    _fields_ = [
        ("s_in", ctypes.c_float), ("n1", LnParams), ("qkv", LinParams),
        ("dy_qk", Dyadic), ("dy_a", Dyadic), ("relb", ctypes.c_void_p),
        ("s_softmax", ctypes.c_float), ("dy_pv", Dyadic), ("proj", LinParams),
        ("res1_main", Dyadic), ("res1_res", Dyadic),
        ("s_mid", ctypes.c_float), ("n2", LnParams), ("fc1", LinParams), ("s_gelu", ctypes.c_float), ("dy_gelu", Dyadic),
        ("fc2", LinParams), ("res2_main", Dyadic), ("res2_res", Dyadic),
        ("exp_aq", ctypes.c_void_p), ("exp_t", ctypes.c_void_p), ("exp_cls", ctypes.c_void_p),
        ("exp_nc", ctypes.c_int), ("exp_tcount", ctypes.c_int), ("exp_dmin", ctypes.c_int),
    ]


class SwinMerge(ctypes.Structure):
    """struct ivit_swin_merge"""
    _fields_ = [("s_in", ctypes.c_float), ("n", LnParams), ("red", LinParams)]


class SwinParams(ctypes.Structure):
    """struct ivit_swin_params"""
    _fields_ = [
        ("pe", LinParams), ("s_bn", ctypes.c_float), ("pn", LnParams), ("dy_qact1", ctypes.c_void_p),
        ("blocks_host", ctypes.POINTER(SwinBlock)), ("merges_host", ctypes.POINTER(SwinMerge)),
        ("s_norm_in", ctypes.c_float), ("n", LnParams), ("dy_pool", Dyadic),
        ("head_w", ctypes.c_void_p), ("head_b", ctypes.c_void_p), ("s_pool", ctypes.c_float),
    ]


_P = ctypes.c_void_p
_I = ctypes.c_int
_L = ctypes.c_int64
_F = ctypes.c_float

# name -> argtypes (all return int status); mirrors include/ivit.h
SIGNATURES = {
    "ivit_create": [ctypes.POINTER(_P), _I, _P],
    "ivit_destroy": [_P],
    "ivit_set_stream": [_P, _P],
    "ivit_set_cu_share": [_P, ctypes.c_int],
    "ivit_quantize_input_f32": [_P, _P, _F, _P, _L],
    "ivit_normalize_quantize_u8": [_P, _P, _I, _I, _I, ctypes.POINTER(_F), ctypes.POINTER(_F), _F, _P],
    "ivit_resize_center_crop_u8": [_P, _P, _I, _I, _I, _I, _I, _P, _P],
    "ivit_requant_i16": [_P, _P, _P, _I, _P, _P, _I, _P, _L, _I],
    "ivit_layernorm_tokenorder_requant": [_P, _P, _L, _I, _F, _P, _P, _P, _I, _P],
    "ivit_patch_norm_tokenorder": [_P, _P, _L, _I, _F, _P, _P, _P, Dyadic, _I, _P],
    "ivit_window_attention_fused": [_P, _P, Dyadic, Dyadic, _P, _F, Dyadic, _P, _I, _I, _I, _I, _I, _I],
    "ivit_window_attention_fused_lut": [_P, _P, Dyadic, Dyadic, _P, _F, _P, _P, _P, _I, _I, _I, Dyadic, _P, _I, _I, _I, _I, _I, _I],
    "ivit_mlp_plan_create": [_P, _P, _P, ctypes.POINTER(_P)],
    "ivit_mlp_fused_planned": [_P, _P, _P, _P, Dyadic, Dyadic, _P, _P, _L],
    "ivit_layernorm_mlp_fused_planned": [_P, _P, _P, _F, _P, _P, _P, _P, _P, Dyadic, Dyadic, _P, _L],
    "ivit_layernorm_mlp_lockstep_planned": [_P, _P, _P, _F, _P, _P, _P, _P, Dyadic, Dyadic, _P, _L],
    "ivit_mlp_fused": [_P, _P, _P, _P, _P, _P, _P, _P, _P, Dyadic, Dyadic, _P, _P, _L, _I, _I],
    "ivit_patch_merge_gather": [_P, _P, _I, _I, _I, _I, _P],
    "ivit_widen_i8_i16": [_P, _P, _P, _L],
    "ivit_linear_i8_requant8_store16": [_P, _P, _P, _P, _P, _P, _I, _I, _I],
    "ivit_patch_merge_layernorm_requant": [_P, _P, _I, _I, _I, _F, _P, _P, _P, _P],
    "ivit_swin_create": [_P, ctypes.POINTER(SwinConfigC), ctypes.POINTER(SwinParams), _I, ctypes.POINTER(_P)],
    "ivit_swin_destroy": [_P],
    "ivit_swin_workspace_bytes": [_P, _I, _I, ctypes.POINTER(ctypes.c_size_t)],
    "ivit_swin_forward": [_P, _P, _I, _I, _P, ctypes.c_size_t, _P],
    "ivit_swin_graph_create": [_P, _P, _I, _I, _P, ctypes.c_size_t, _P, ctypes.POINTER(_P)],
    "ivit_vit_create": [_P, ctypes.POINTER(VitConfig), ctypes.POINTER(VitParams), _I, ctypes.POINTER(_P)],
    "ivit_vit_destroy": [_P],
    "ivit_vit_workspace_bytes": [_P, _I, _I, ctypes.POINTER(ctypes.c_size_t)],
    "ivit_vit_fused_mlp_blocks": [_P, _I, ctypes.POINTER(_I)],
    "ivit_vit_fused_ln_mlp_blocks": [_P, _I, ctypes.POINTER(_I)],
    "ivit_vit_fused_qkv_blocks": [_P, _I, ctypes.POINTER(_I)],
    "ivit_vit_cls_tail": [_P, _I, ctypes.POINTER(_I)],
    "ivit_swin_fused_mlp_blocks": [_P, _I, ctypes.POINTER(_I * 4)],
    "ivit_vit_workspace_init": [_P, _P, ctypes.c_size_t, _I, _I],
    "ivit_vit_forward": [_P, _P, _I, _I, _P, ctypes.c_size_t, _P],
    "ivit_vit_graph_create": [_P, _P, _I, _I, _P, ctypes.c_size_t, _P, ctypes.POINTER(_P)],
    "ivit_graph_launch": [_P],
    "ivit_graph_destroy": [_P],
    "ivit_linear_i8": [_P, _P, _P, _P, _P, _I, _I, _I],
    "ivit_linear_i8_requant": [_P, _P, _P, _P, _P, _I, _P, _I, _I, _I],
    "ivit_linear_i8_requant_residual": [_P, _P, _P, _P, _P, Dyadic, Dyadic, _P, _P, _I, _I, _I],
    "ivit_linear_i8_qkv": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I],
    "ivit_constants_upload": [_P, _P, ctypes.c_size_t, _P],
    "ivit_constants_broadcast": [_P, _P, ctypes.c_size_t, _I, _P],
    "ivit_linear_plan_create": [_P, _P, _P, _P, _I, _I, ctypes.POINTER(_P)],
    "ivit_linear_i8_requant_planned": [_P, _P, _P, _I, _P, _I],
    "ivit_linear_i8_requant_residual_planned": [_P, _P, _P, Dyadic, Dyadic, _P, _P, _I],
    "ivit_linear_i8_qkv_planned": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I],
    "ivit_linear_plan_prepare_ws": [_P, _P],
    "ivit_layernorm_linear_i8_requant_planned": [_P, _P, _P, _F, _P, _P, _P, _P, _I],
    "ivit_linear_i8_requant_residual_layernorm_planned": [_P, _P, _P, Dyadic, Dyadic, _P, _P, _I, _F, _P, _P, _P, _P],
    "ivit_layernorm_linear_i8_qkv_planned": [_P, _P, _P, _F, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I],
    "ivit_layernorm_linear_i8_qkv_ldv_planned": [_P, _P, _P, _F, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I],
    "ivit_bmm_nt_i8": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _L, _L, _L],
    "ivit_bmm_nt_u16i8": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _L, _L, _L],
    "ivit_attn_qk_requant": [_P, _P, _P, Dyadic, _P, _I, _I, _I, _I],
    "ivit_attn_pv_requant": [_P, _P, _P, Dyadic, _P, _I, _I, _I, _I, _I, _I],
    "ivit_attention_fused": [_P, _P, _P, _P, Dyadic, _F, Dyadic, _P, _I, _I, _I, _I, _I],
    "ivit_attention_fused_lut": [_P, _P, _P, _P, Dyadic, _F, _P, _P, _P, _I, _I, _I, Dyadic, _P, _I, _I, _I, _I, _I],
    "ivit_shiftmax_rowtable": [_P, _P, _P, _P, _I, _I, _I, _P],
    "ivit_attention_fused_rowlut": [_P, _P, _P, _P, Dyadic, _F, _P, _I, Dyadic, _P, _I, _I, _I, _I, _I],
    "ivit_attention_fused_cls": [_P, _P, _P, _P, Dyadic, _F, Dyadic, _P, _P, _P, _I, _I, _I, _I, _I],
    "ivit_attention_fused_lut_cls": [_P, _P, _P, _P, Dyadic, _F, _P, _P, _P, _I, _I, _I, Dyadic, _P, _P, _P, _I, _I, _I, _I, _I],
    "ivit_attention_fused_rowlut_cls": [_P, _P, _P, _P, Dyadic, _F, _P, _I, Dyadic, _P, _P, _P, _I, _I, _I, _I, _I],
    "ivit_gather_rows_i16": [_P, _P, _L, _I, _L, _P],
    "ivit_requant_i32": [_P, _P, _P, _I, _P, _P, _I, _P, _L, _I],
    "ivit_requant_f32": [_P, _P, _P, _I, _P, _P, _I, _P, _L, _I],
    "ivit_shiftmax": [_P, _P, _L, _I, _I, _F, _I, _P, _I],
    "ivit_shiftgelu": [_P, _P, _L, _I, _F, _P],
    "ivit_shiftgelu_requant": [_P, _P, _L, _I, _F, Dyadic, _P],
    "ivit_shiftgelu_build_table": [_P, _F, Dyadic, _P],
    "ivit_shiftgelu_requant_lut": [_P, _P, _L, _I, _P, _P],
    "ivit_layernorm": [_P, _P, _L, _I, _F, _P, _P, _P],
    "ivit_layernorm_requant": [_P, _P, _L, _I, _L, _F, _P, _P, _P, _P],
    "ivit_shiftmax_masked": [_P, _P, _L, _I, _I, _F, _I, _P, _I, _I, _P, _I],
    "ivit_requant_i32_bcast": [_P, _P, Dyadic, _P, _L, Dyadic, _I, _P, _L],
    "ivit_avgpool_requant": [_P, _P, _I, _I, _I, Dyadic, _P],
    "ivit_avgpool_requant_scaled": [_P, _P, _I, _I, _I, _F, Dyadic, _P],
    "ivit_layernorm_tokenorder": [_P, _P, _L, _I, _F, _P, _P, _I, _P],
    "ivit_debug_div": [_P, _P, _P, _P, _P, _L],
    "ivit_debug_requotient": [_P, _P, _P, _P, _P, _L],
    "ivit_im2col_patch": [_P, _P, _I, _I, _I, _I, _I, _P],
    "ivit_embed_finish": [_P, _P, _P, _P, Dyadic, Dyadic, _P, _I, _I, _I],
    "ivit_patch_embed": [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, Dyadic, Dyadic, _P, _I],
    "ivit_logits_topk": [_P, _P, _P, _I, _I, _I, _P, _P],
    "ivit_vit_predict": [_P, _P, _I, _I, _P, ctypes.c_size_t, _P, _P, _I, _P, _P],
    "ivit_swin_predict": [_P, _P, _I, _I, _P, ctypes.c_size_t, _P, _P, _I, _P, _P],
    "ivit_vit_predict_graph_create": [_P, _P, _I, _I, _P, ctypes.c_size_t, _P, _P, _I, _P, _P, ctypes.POINTER(_P)],
    "ivit_swin_predict_graph_create": [_P, _P, _I, _I, _P, ctypes.c_size_t, _P, _P, _I, _P, _P, ctypes.POINTER(_P)],
}


class ImageDesc(ctypes.Structure):
    """struct ivit_image_desc: image i of a ragged batch is h * w * 3 bytes at pixels + offset, uint8 HWC"""
    _fields_ = [("offset", ctypes.c_int64), ("h", ctypes.c_int32), ("w", ctypes.c_int32)]


# The PIL-pinned ragged front end (include/ivit.h; csrc/ivit_preprocess.h), bound like SIGNATURES and walked by load() in the same
# way.  A table of its own: tests/abi_cases.py holds one case per name of SIGNATURES in the shape its twin tables know, and these
# entries take a host AND a device descriptor table; their memory contract is tested in tests/test_pil_resize_gpu.py on the same
# arena harness.
_D = ctypes.POINTER(ImageDesc)
FRONT_END_SIGNATURES = {
    "ivit_resize_center_crop_u8_pil": [_P, _P, ctypes.c_size_t, _D, _P, _I, _I, _I, _P],
    "ivit_eval_transform_u8": [_P, _P, ctypes.c_size_t, _D, _P, _I, _I, _I, ctypes.POINTER(_F), ctypes.POINTER(_F), _F, _P],
}
OTHER_SYMBOLS = ["ivit_version", "ivit_status_string", "ivit_last_error", "ivit_linear_plan_destroy", "ivit_mlp_plan_destroy", "ivit_linear_plan_query", "ivit_mlp_plan_select"]

_lib = None


def load():
    """dlopen the in-tree library; raises IvitError if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise IvitError(f"{SO_PATH} not built — run `python -c 'import __graft_entry__ as g; g.build()'`; "
                        "there is no CPU fallback for the product path")
    lib = ctypes.CDLL(SO_PATH)
    for table in (SIGNATURES, FRONT_END_SIGNATURES):
        for name, args in table.items():
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = ctypes.c_int
    lib.ivit_version.restype = ctypes.c_int
    lib.ivit_status_string.restype = ctypes.c_char_p
    lib.ivit_status_string.argtypes = [ctypes.c_int]
    lib.ivit_last_error.restype = ctypes.c_char_p
    lib.ivit_last_error.argtypes = [_P]
    lib.ivit_linear_plan_destroy.argtypes = [_P]
    lib.ivit_linear_plan_destroy.restype = ctypes.c_int
    lib.ivit_linear_plan_query.argtypes = [_P, ctypes.POINTER(_I), ctypes.POINTER(_I)]
    lib.ivit_linear_plan_query.restype = ctypes.c_int
    lib.ivit_mlp_plan_select.argtypes = [_P, _I]
    lib.ivit_mlp_plan_select.restype = ctypes.c_int
    lib.ivit_mlp_plan_destroy.argtypes = [_P]
    lib.ivit_mlp_plan_destroy.restype = ctypes.c_int
    _lib = lib
    return lib


class Handle:
    """ivit_handle bound to (device, HIP stream)."""

    def __init__(self, device=0, stream=None):
        self.lib = load()
        h = _P()
        st = self.lib.ivit_create(ctypes.byref(h), int(device), _P(stream or 0))
        if st != 0:
            raise IvitError(f"ivit_create(device={device}): {self.lib.ivit_status_string(st).decode()}")
        self.h = h
        self.device = device

    def set_stream(self, stream):
        self._check(self.lib.ivit_set_stream(self.h, _P(stream or 0)), "ivit_set_stream")

    def set_cu_share(self, cus):
        """CUs the one-workgroup-per-CU kernels launched through this handle size their grids for (0 = the whole device): a
        caller running several handles side by side on slices of a batch gives each its share (include/ivit.h)."""
        self._check(self.lib.ivit_set_cu_share(self.h, int(cus)), "ivit_set_cu_share")

    def _check(self, st, name):
        if st != 0:
            raise IvitError(f"{name}: {self.lib.ivit_status_string(st).decode()} "
                            f"({self.lib.ivit_last_error(self.h).decode()})")

    def call(self, name, *args):
        self._check(getattr(self.lib, name)(self.h, *args), name)

    def try_call(self, name, *args):
        """call(), but IVIT_ERR_UNSUPPORTED (the entry point refused the shape and launched nothing) returns False instead of raising."""
        self.unsupported = False

        def check(st, nm):
            if st == IVIT_ERR_UNSUPPORTED:
                self.unsupported = True
            else:
                self._check_plain(st, nm)
        self._check_plain, self._check = self._check, check
        try:
            self.call(name, *args)          # through self.call: a timing wrapper installed on it sees this launch too
        finally:
            self._check = self._check_plain
        return not self.unsupported

    def linear_plan(self, w, bias, dy, N, K):
        """ivit_linear_plan_create: returns a LinearPlan (frozen QuantLinear: w/bias/dy device pointers must outlive it)."""
        return LinearPlan(self, w, bias, dy, N, K)

    def close(self):
        if self.h:
            self.lib.ivit_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LinearPlan:
    """ivit_linear_plan: per-channel multipliers + exactness bounds of one frozen QuantLinear (include/ivit.h)."""

    def __init__(self, handle, w, bias, dy, N, K):
        self.lib = handle.lib
        p = _P()
        handle._check(self.lib.ivit_linear_plan_create(handle.h, w, bias, dy, int(N), int(K), ctypes.byref(p)),
                      "ivit_linear_plan_create")
        self.p = p
        a, b = _I(0), _I(0)
        self.lib.ivit_linear_plan_query(p, ctypes.byref(a), ctypes.byref(b))
        self.pipelined_ok, self.single_fma_ok = bool(a.value), bool(b.value)

    def close(self):
        if self.p:
            self.lib.ivit_linear_plan_destroy(self.p)
            self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
