"""Width 192 on the weights-in-registers GEMM without a GPU to run it: the C ABI's additions are declared, bound and exported with the
same argument counts, the K = 192 instantiations are in the gfx950 code object, and the fragment order the weights are rewritten into
is a permutation of the weight bytes."""
import os
import re
import struct

import numpy as np
import pytest

import ivit_amd as iv
from ivit_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ivit_layernorm_linear_i8_qkv_ldv_planned", "ivit_vit_fused_qkv_blocks")


def _prototype_args(name):
    hdr = open(os.path.join(ROOT, "include", "ivit.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, hdr, flags=re.S)
    assert m, "include/ivit.h has no prototype for " + name
    return [a.strip() for a in m.group(1).split(",")]


def test_ws192_entries_declared_bound_and_exported():
    lib = _lib.load()
    for name in NEW:
        args = _prototype_args(name)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name]) == len(args), (name, args)
    # the new entry is the existing one with ldv behind it
    old, new = _prototype_args("ivit_layernorm_linear_i8_qkv_planned"), _prototype_args(NEW[0])
    assert len(new) == len(old) + 1 and new[-1] == "int ldv"
    assert _lib.SIGNATURES[NEW[0]][:-1] == _lib.SIGNATURES["ivit_layernorm_linear_i8_qkv_planned"]
    hdr = open(os.path.join(ROOT, "include", "ivit.h")).read()
    assert int(re.search(r"#define IVIT_VERSION (\d+)", hdr).group(1)) >= 110
    assert lib.ivit_version() >= 110


def _device_code_object(so_path):
    """The gfx950 ELF inside the library's clang offload bundle (.hip_fatbin)."""
    b = open(so_path, "rb").read()
    i = b.find(b"__CLANG_OFFLOAD_BUNDLE__")
    assert i >= 0, "no offload bundle in the library"
    n = struct.unpack_from("<Q", b, i + 24)[0]
    off = i + 32
    for _ in range(n):
        o, sz, t = struct.unpack_from("<QQQ", b, off)
        off += 24
        name = b[off:off + t].decode()
        off += t
        if "gfx950" in name:
            return b[i + o:i + o + sz]
    raise AssertionError("no gfx950 code object")


def test_ws192_kernels_compiled_for_gfx950():
    """Both geometries of gemm_ws_qkv_kernel; at K = 192 every epilogue (0 qkv scatter, 1 proj + residual, 2 plain 8-bit) in both requant
    forms, the LayerNorm head on the two 8-bit ones, and the v^T store form of the scatter."""
    co = _device_code_object(iv.build())
    names = set(re.findall(rb"_Z18gemm_ws_qkv_kernelI5WsGeoILi(\d+)ELi\d+ELb[01]EELb([01])ELb([01])ELi(\d)ELb([01])EEv6WsArgs", co))
    for fma in (b"0", b"1"):
        for epi, lns, vts in ((b"0", (b"0", b"1"), (b"0", b"1")), (b"2", (b"0", b"1"), (b"0",)), (b"1", (b"0",), (b"0",))):
            for ln in lns:
                for vt in vts:
                    assert (b"192", fma, ln, epi, vt) in names, (fma, ln, epi, vt)
        assert (b"384", fma, b"1", b"0", b"0") in names and (b"384", fma, b"1", b"1", b"0") in names
    assert not any(n[0] == b"384" and n[4] == b"1" for n in names)       # no v^T form at 384


def ws_fragment_order(N, K):
    """ws_swizzle_kernel's index map restated: 16-byte unit i of the fragment-ordered copy -> (weight row, first column).  Unit i is lane
    l = i % 64 of fragment f = i // 64 = ct * (K / 32) + ks: the 32 rows of channel tile ct in the order that makes accumulator register v
    of lane (token, h) channel 16 h + v, the 32 columns of k-step ks as two halves."""
    i = np.arange(N * K // 16)
    l, f = i & 63, i >> 6
    ct, ks = f // (K // 32), f % (K // 32)
    rho = l & 31
    ch = 32 * ct + ((rho >> 2) & 1) * 16 + (rho >> 3) * 4 + (rho & 3)
    return ch, 32 * ks + 16 * (l >> 5)


@pytest.mark.parametrize("N", [192, 576, 768])
def test_ws192_fragment_order_is_a_bijection(N):
    K = 192
    ch, col = ws_fragment_order(N, K)
    src = (ch[:, None] * K + col[:, None] + np.arange(16)[None, :]).ravel()
    assert src.size == N * K and src.min() == 0 and src.max() == N * K - 1
    assert np.array_equal(np.sort(src), np.arange(N * K))
    # a 64-channel slab is one contiguous run of 2 * K / 32 fragments: what a wave loads into its registers
    slab = ch[: 2 * (K // 32) * 64]
    assert set(slab.tolist()) == set(range(64))
