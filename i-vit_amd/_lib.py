"""ctypes binding of the C-ABI in include/ivit.h, include/ivit_eval.h, include/ivit_features.h, include/ivit_attnmap.h, include/ivit_classmap.h, include/ivit_hidden.h, include/ivit_search.h, include/ivit_modelfile.h, include/ivit_probe.h, include/ivit_views.h, include/ivit_cluster.h, include/ivit_range.h and include/ivit_jpeg.h (libivit_hip.so, built in-tree).  Nothing of the ABI is
restated here: the Structures, the status codes and every argtypes / restype are derived from the headers by _abi.py (the mapping
rule is stated there).  ivit.h is frozen at IVIT_VERSION 111: ABI / SIGNATURES / RESTYPES are its prototypes and stay what they are;
the entries that came after it are those of ivit_eval.h, under EVAL_ABI / EVAL_SIGNATURES / EVAL_RESTYPES, of ivit_features.h,
under FEATURES_ABI / FEATURES_SIGNATURES / FEATURES_RESTYPES, of ivit_attnmap.h, under ATTNMAP_ABI / ATTNMAP_SIGNATURES /
ATTNMAP_RESTYPES, of ivit_classmap.h, under CLASSMAP_ABI / CLASSMAP_SIGNATURES / CLASSMAP_RESTYPES, of ivit_hidden.h, under
HIDDEN_ABI / HIDDEN_SIGNATURES / HIDDEN_RESTYPES, of ivit_search.h, under SEARCH_ABI / SEARCH_SIGNATURES / SEARCH_RESTYPES, of
ivit_modelfile.h, under MODELFILE_ABI / MODELFILE_SIGNATURES / MODELFILE_RESTYPES, of ivit_probe.h, under PROBE_ABI /
PROBE_SIGNATURES / PROBE_RESTYPES, of ivit_views.h, under VIEWS_ABI / VIEWS_SIGNATURES / VIEWS_RESTYPES, of ivit_cluster.h, under CLUSTER_ABI /
CLUSTER_SIGNATURES / CLUSTER_RESTYPES, of ivit_range.h, under RANGE_ABI / RANGE_SIGNATURES / RANGE_RESTYPES, and of ivit_jpeg.h, under JPEG_ABI /
JPEG_SIGNATURES / JPEG_RESTYPES (its struct ivit_jpeg_desc is JpegDesc).

The product path has NO CPU fallback: if the HIP library is missing or a call
fails, an exception is raised.
"""
import ctypes
import os
import subprocess

from . import _abi

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
# gfx950 only, SRAM-ECC on (the only mode MI355X ships in): ivit_wa.h (wa_gelu_issue: ivit_mlp_rs.h, ivit_swin_mlp_rs.h) relies on ds_read_u8_d16_hi ZEROING the low
# half of its destination, which is the d16 behaviour of SRAM-ECC parts; a target without it would need the merge written out.
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-pass-failed", "-fPIC", "-shared",
               "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]


ABI = _abi.ABI
IVIT_VERSION = ABI.constants["IVIT_VERSION"]
IVIT_OK, IVIT_ERR_INVALID, IVIT_ERR_HIP, IVIT_ERR_UNSUPPORTED, IVIT_ERR_NO_DEVICE = (
    ABI.constants[n] for n in ("IVIT_OK", "IVIT_ERR_INVALID", "IVIT_ERR_HIP", "IVIT_ERR_UNSUPPORTED", "IVIT_ERR_NO_DEVICE"))

# struct of the header -> its name here.  Pointer members are c_void_p: assign an address (ctypes.addressof(array)) and keep the
# array alive yourself.
STRUCT_NAMES = {"ivit_dyadic": "Dyadic", "ivit_image_desc": "ImageDesc", "ivit_vit_config": "VitConfig", "ivit_vit_block": "VitBlock",
                "ivit_vit_params": "VitParams", "ivit_ln_params": "LnParams", "ivit_lin_params": "LinParams",
                "ivit_swin_config": "SwinConfigC", "ivit_swin_block": "SwinBlock", "ivit_swin_merge": "SwinMerge",
                "ivit_swin_params": "SwinParams"}
assert set(STRUCT_NAMES) == set(ABI.structs), set(STRUCT_NAMES) ^ set(ABI.structs)
_structs = _abi.structures(ABI, STRUCT_NAMES)
globals().update((STRUCT_NAMES[n], cls) for n, cls in _structs.items())

_signatures = _abi.signatures(ABI, _structs)
RESTYPES = {name: ret for name, (ret, args) in _signatures.items()}        # prototype of the header -> restype
SIGNATURES = {name: args for name, (ret, args) in _signatures.items()}      # prototype of the header -> argtypes

# include/ivit_eval.h, by the same rule (it declares no struct of its own: the Structures are those of ivit.h)
EVAL_ABI = _abi.EVAL_ABI
IVIT_EVAL_VERSION = EVAL_ABI.constants["IVIT_EVAL_VERSION"]
assert set(EVAL_ABI.structs) == set(ABI.structs) and not set(EVAL_ABI.functions) & set(ABI.functions)
_eval_signatures = _abi.signatures(EVAL_ABI, _structs)
EVAL_RESTYPES = {name: ret for name, (ret, args) in _eval_signatures.items()}
EVAL_SIGNATURES = {name: args for name, (ret, args) in _eval_signatures.items()}

# include/ivit_features.h, likewise
FEATURES_ABI = _abi.FEATURES_ABI
IVIT_FEATURES_VERSION, IVIT_FEATURES_DEQUANT, IVIT_FEATURES_UNIT = (
    FEATURES_ABI.constants[n] for n in ("IVIT_FEATURES_VERSION", "IVIT_FEATURES_DEQUANT", "IVIT_FEATURES_UNIT"))
assert set(FEATURES_ABI.structs) == set(ABI.structs) and not set(FEATURES_ABI.functions) & (set(ABI.functions) | set(EVAL_ABI.functions))
_features_signatures = _abi.signatures(FEATURES_ABI, _structs)
FEATURES_RESTYPES = {name: ret for name, (ret, args) in _features_signatures.items()}
FEATURES_SIGNATURES = {name: args for name, (ret, args) in _features_signatures.items()}

# include/ivit_attnmap.h, likewise
ATTNMAP_ABI = _abi.ATTNMAP_ABI
IVIT_ATTNMAP_VERSION, IVIT_ATTNMAP_HEADS, IVIT_ATTNMAP_MEAN = (
    ATTNMAP_ABI.constants[n] for n in ("IVIT_ATTNMAP_VERSION", "IVIT_ATTNMAP_HEADS", "IVIT_ATTNMAP_MEAN"))
assert set(ATTNMAP_ABI.structs) == set(ABI.structs) and not set(ATTNMAP_ABI.functions) & (
    set(ABI.functions) | set(EVAL_ABI.functions) | set(FEATURES_ABI.functions))
_attnmap_signatures = _abi.signatures(ATTNMAP_ABI, _structs)
ATTNMAP_RESTYPES = {name: ret for name, (ret, args) in _attnmap_signatures.items()}
ATTNMAP_SIGNATURES = {name: args for name, (ret, args) in _attnmap_signatures.items()}

# include/ivit_classmap.h, likewise
CLASSMAP_ABI = _abi.CLASSMAP_ABI
IVIT_CLASSMAP_VERSION, IVIT_CLASSMAP_TOPK, IVIT_CLASSMAP_GIVEN = (
    CLASSMAP_ABI.constants[n] for n in ("IVIT_CLASSMAP_VERSION", "IVIT_CLASSMAP_TOPK", "IVIT_CLASSMAP_GIVEN"))
assert set(CLASSMAP_ABI.structs) == set(ABI.structs) and not set(CLASSMAP_ABI.functions) & (
    set(ABI.functions) | set(EVAL_ABI.functions) | set(FEATURES_ABI.functions) | set(ATTNMAP_ABI.functions))
_classmap_signatures = _abi.signatures(CLASSMAP_ABI, _structs)
CLASSMAP_RESTYPES = {name: ret for name, (ret, args) in _classmap_signatures.items()}
CLASSMAP_SIGNATURES = {name: args for name, (ret, args) in _classmap_signatures.items()}

# include/ivit_hidden.h, likewise
HIDDEN_ABI = _abi.HIDDEN_ABI
IVIT_HIDDEN_VERSION, IVIT_HIDDEN_TOKENS, IVIT_HIDDEN_GRID = (
    HIDDEN_ABI.constants[n] for n in ("IVIT_HIDDEN_VERSION", "IVIT_HIDDEN_TOKENS", "IVIT_HIDDEN_GRID"))
assert set(HIDDEN_ABI.structs) == set(ABI.structs) and not set(HIDDEN_ABI.functions) & (
    set(ABI.functions) | set(EVAL_ABI.functions) | set(FEATURES_ABI.functions) | set(ATTNMAP_ABI.functions) | set(CLASSMAP_ABI.functions))
_hidden_signatures = _abi.signatures(HIDDEN_ABI, _structs)
HIDDEN_RESTYPES = {name: ret for name, (ret, args) in _hidden_signatures.items()}
HIDDEN_SIGNATURES = {name: args for name, (ret, args) in _hidden_signatures.items()}

# include/ivit_search.h, likewise
SEARCH_ABI = _abi.SEARCH_ABI
IVIT_SEARCH_VERSION = SEARCH_ABI.constants["IVIT_SEARCH_VERSION"]
assert set(SEARCH_ABI.structs) == set(ABI.structs) and not set(SEARCH_ABI.functions) & (
    set(ABI.functions) | set(EVAL_ABI.functions) | set(FEATURES_ABI.functions) | set(ATTNMAP_ABI.functions) | set(CLASSMAP_ABI.functions)
    | set(HIDDEN_ABI.functions))
_search_signatures = _abi.signatures(SEARCH_ABI, _structs)
SEARCH_RESTYPES = {name: ret for name, (ret, args) in _search_signatures.items()}
SEARCH_SIGNATURES = {name: args for name, (ret, args) in _search_signatures.items()}

# include/ivit_modelfile.h, likewise; it declares one struct of its own, ivit_model_info (ModelInfo here), beside those of ivit.h
MODELFILE_ABI = _abi.MODELFILE_ABI
IVIT_MODELFILE_VERSION = MODELFILE_ABI.constants["IVIT_MODELFILE_VERSION"]
assert set(MODELFILE_ABI.structs) == set(ABI.structs) | {"ivit_model_info"} and not set(MODELFILE_ABI.functions) & (
    set(ABI.functions) | set(EVAL_ABI.functions) | set(FEATURES_ABI.functions) | set(ATTNMAP_ABI.functions) | set(CLASSMAP_ABI.functions)
    | set(HIDDEN_ABI.functions) | set(SEARCH_ABI.functions))
_modelfile_structs = dict(_structs)
_modelfile_structs.update((n, c) for n, c in _abi.structures(MODELFILE_ABI, dict(STRUCT_NAMES, ivit_model_info="ModelInfo")).items()
                          if n not in _structs)
ModelInfo = _modelfile_structs["ivit_model_info"]
_modelfile_signatures = _abi.signatures(MODELFILE_ABI, _modelfile_structs)
MODELFILE_RESTYPES = {name: ret for name, (ret, args) in _modelfile_signatures.items()}
MODELFILE_SIGNATURES = {name: args for name, (ret, args) in _modelfile_signatures.items()}

# include/ivit_probe.h, by the rule of ivit_search.h
PROBE_ABI = _abi.PROBE_ABI
IVIT_PROBE_VERSION = PROBE_ABI.constants["IVIT_PROBE_VERSION"]
assert set(PROBE_ABI.structs) == set(ABI.structs) and not set(PROBE_ABI.functions) & (
    set(ABI.functions) | set(EVAL_ABI.functions) | set(FEATURES_ABI.functions) | set(ATTNMAP_ABI.functions) | set(CLASSMAP_ABI.functions)
    | set(HIDDEN_ABI.functions) | set(SEARCH_ABI.functions) | set(MODELFILE_ABI.functions))
_probe_signatures = _abi.signatures(PROBE_ABI, _structs)
PROBE_RESTYPES = {name: ret for name, (ret, args) in _probe_signatures.items()}
PROBE_SIGNATURES = {name: args for name, (ret, args) in _probe_signatures.items()}

# include/ivit_views.h, by the rule of ivit_modelfile.h: it declares one struct of its own, ivit_view_desc (ViewDesc here)
VIEWS_ABI = _abi.VIEWS_ABI
IVIT_VIEWS_VERSION = VIEWS_ABI.constants["IVIT_VIEWS_VERSION"]
assert set(VIEWS_ABI.structs) == set(ABI.structs) | {"ivit_view_desc"} and not set(VIEWS_ABI.functions) & (
    set(ABI.functions) | set(EVAL_ABI.functions) | set(FEATURES_ABI.functions) | set(ATTNMAP_ABI.functions) | set(CLASSMAP_ABI.functions)
    | set(HIDDEN_ABI.functions) | set(SEARCH_ABI.functions) | set(MODELFILE_ABI.functions) | set(PROBE_ABI.functions))
_views_structs = dict(_structs)
_views_structs.update((n, c) for n, c in _abi.structures(VIEWS_ABI, dict(STRUCT_NAMES, ivit_view_desc="ViewDesc")).items() if n not in _structs)
ViewDesc = _views_structs["ivit_view_desc"]
_views_signatures = _abi.signatures(VIEWS_ABI, _views_structs)
VIEWS_RESTYPES = {name: ret for name, (ret, args) in _views_signatures.items()}
VIEWS_SIGNATURES = {name: args for name, (ret, args) in _views_signatures.items()}

# include/ivit_cluster.h, by the rule of ivit_probe.h
CLUSTER_ABI = _abi.CLUSTER_ABI
IVIT_CLUSTER_VERSION = CLUSTER_ABI.constants["IVIT_CLUSTER_VERSION"]
assert set(CLUSTER_ABI.structs) == set(ABI.structs) and not set(CLUSTER_ABI.functions) & (
    set(ABI.functions) | set(EVAL_ABI.functions) | set(FEATURES_ABI.functions) | set(ATTNMAP_ABI.functions) | set(CLASSMAP_ABI.functions)
    | set(HIDDEN_ABI.functions) | set(SEARCH_ABI.functions) | set(MODELFILE_ABI.functions) | set(PROBE_ABI.functions) | set(VIEWS_ABI.functions))
_cluster_signatures = _abi.signatures(CLUSTER_ABI, _structs)
CLUSTER_RESTYPES = {name: ret for name, (ret, args) in _cluster_signatures.items()}
CLUSTER_SIGNATURES = {name: args for name, (ret, args) in _cluster_signatures.items()}

# include/ivit_range.h, by the rule of ivit_probe.h
RANGE_ABI = _abi.RANGE_ABI
IVIT_RANGE_VERSION = RANGE_ABI.constants["IVIT_RANGE_VERSION"]
assert set(RANGE_ABI.structs) == set(ABI.structs) and not set(RANGE_ABI.functions) & (
    set(ABI.functions) | set(EVAL_ABI.functions) | set(FEATURES_ABI.functions) | set(ATTNMAP_ABI.functions) | set(CLASSMAP_ABI.functions)
    | set(HIDDEN_ABI.functions) | set(SEARCH_ABI.functions) | set(MODELFILE_ABI.functions) | set(PROBE_ABI.functions) | set(VIEWS_ABI.functions)
    | set(CLUSTER_ABI.functions))
_range_signatures = _abi.signatures(RANGE_ABI, _structs)
RANGE_RESTYPES = {name: ret for name, (ret, args) in _range_signatures.items()}
RANGE_SIGNATURES = {name: args for name, (ret, args) in _range_signatures.items()}

# include/ivit_jpeg.h, by the rule of ivit_views.h: it declares one struct of its own, ivit_jpeg_desc (JpegDesc here)
JPEG_ABI = _abi.JPEG_ABI
IVIT_JPEG_VERSION = JPEG_ABI.constants["IVIT_JPEG_VERSION"]
assert set(JPEG_ABI.structs) == set(ABI.structs) | {"ivit_jpeg_desc"} and not set(JPEG_ABI.functions) & (
    set(ABI.functions) | set(EVAL_ABI.functions) | set(FEATURES_ABI.functions) | set(ATTNMAP_ABI.functions) | set(CLASSMAP_ABI.functions)
    | set(HIDDEN_ABI.functions) | set(SEARCH_ABI.functions) | set(MODELFILE_ABI.functions) | set(PROBE_ABI.functions) | set(VIEWS_ABI.functions)
    | set(CLUSTER_ABI.functions) | set(RANGE_ABI.functions))
_jpeg_structs = dict(_structs)
_jpeg_structs.update((n, c) for n, c in _abi.structures(JPEG_ABI, dict(STRUCT_NAMES, ivit_jpeg_desc="JpegDesc")).items() if n not in _structs)
JpegDesc = _jpeg_structs["ivit_jpeg_desc"]
_jpeg_signatures = _abi.signatures(JPEG_ABI, _jpeg_structs)
JPEG_RESTYPES = {name: ret for name, (ret, args) in _jpeg_signatures.items()}
JPEG_SIGNATURES = {name: args for name, (ret, args) in _jpeg_signatures.items()}


class IvitError(RuntimeError):
    pass


def build(force=False, verbose=False):
    """Compile the HIP extension for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(_CSRC, s) for s in SOURCES]
    newest = max(os.path.getmtime(p) for p in srcs + [_abi.HEADER, _abi.EVAL_HEADER, _abi.FEATURES_HEADER, _abi.ATTNMAP_HEADER, _abi.CLASSMAP_HEADER, _abi.HIDDEN_HEADER, _abi.SEARCH_HEADER, _abi.MODELFILE_HEADER, _abi.PROBE_HEADER, _abi.VIEWS_HEADER, _abi.CLUSTER_HEADER, _abi.RANGE_HEADER, _abi.JPEG_HEADER, _THIS])      # the flags live in this file
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


_P = ctypes.c_void_p
_I = ctypes.c_int


def bind(lib, names=None, prefix="ivit_"):
    """sets argtypes and restype of lib.<prefix><name> from the header's prototype of ivit_<name>, for every name in `names`
    (default: every prototype of the header) — for the library itself and for any other that exports the same prototypes under
    another prefix (the CPU twin: prefix="ivit_cpu_").  A missing symbol is an AttributeError."""
    for name in (n[len("ivit_"):] for n in SIGNATURES) if names is None else names:
        fn = getattr(lib, prefix + name)
        fn.argtypes, fn.restype = SIGNATURES["ivit_" + name], RESTYPES["ivit_" + name]
    return lib


def bind_eval(lib):
    """the same for every prototype of include/ivit_eval.h"""
    for name, args in EVAL_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, EVAL_RESTYPES[name]
    return lib


def bind_features(lib):
    """the same for every prototype of include/ivit_features.h"""
    for name, args in FEATURES_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, FEATURES_RESTYPES[name]
    return lib


def bind_attnmap(lib):
    """the same for every prototype of include/ivit_attnmap.h"""
    for name, args in ATTNMAP_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, ATTNMAP_RESTYPES[name]
    return lib


def bind_classmap(lib):
    """the same for every prototype of include/ivit_classmap.h"""
    for name, args in CLASSMAP_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, CLASSMAP_RESTYPES[name]
    return lib


def bind_hidden(lib):
    """the same for every prototype of include/ivit_hidden.h"""
    for name, args in HIDDEN_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, HIDDEN_RESTYPES[name]
    return lib


def bind_search(lib):
    """the same for every prototype of include/ivit_search.h"""
    for name, args in SEARCH_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, SEARCH_RESTYPES[name]
    return lib


def bind_modelfile(lib):
    """the same for every prototype of include/ivit_modelfile.h"""
    for name, args in MODELFILE_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, MODELFILE_RESTYPES[name]
    return lib


def bind_probe(lib):
    """the same for every prototype of include/ivit_probe.h"""
    for name, args in PROBE_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, PROBE_RESTYPES[name]
    return lib


def bind_views(lib):
    """the same for every prototype of include/ivit_views.h"""
    for name, args in VIEWS_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, VIEWS_RESTYPES[name]
    return lib


def bind_cluster(lib):
    """the same for every prototype of include/ivit_cluster.h"""
    for name, args in CLUSTER_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, CLUSTER_RESTYPES[name]
    return lib


def bind_range(lib):
    """the same for every prototype of include/ivit_range.h"""
    for name, args in RANGE_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, RANGE_RESTYPES[name]
    return lib


def bind_jpeg(lib):
    """the same for every prototype of include/ivit_jpeg.h"""
    for name, args in JPEG_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, JPEG_RESTYPES[name]
    return lib


_lib = None


def load():
    """dlopen the in-tree library; raises IvitError if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise IvitError(f"{SO_PATH} not built — run `python -c 'import __graft_entry__ as g; g.build()'`; "
                        "there is no CPU fallback for the product path")
    _lib = bind_jpeg(bind_range(bind_cluster(bind_views(bind_probe(bind_modelfile(bind_search(bind_hidden(bind_classmap(bind_attnmap(bind_features(bind_eval(bind(ctypes.CDLL(SO_PATH))))))))))))))
    return _lib


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
