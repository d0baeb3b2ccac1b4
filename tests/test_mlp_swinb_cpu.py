"""The fused Mlp of Swin-B's stages 0 and 1 (widths 128 and 256) exists in the built library without a GPU to run it: both
kernels are in the gfx950 code object, and header and library say version 108."""
import os
import re
import struct

import ivit_amd as iv
from ivit_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def test_mlp256_and_mlp128_kernels_compiled_for_gfx950():
    co = _device_code_object(iv.build())
    # width 256: both requant forms (single-FMA and multiply-add) and the swizzle kernel of its plan
    assert re.search(rb"_Z\d+mlp256_kernelILb1EE", co) and re.search(rb"_Z\d+mlp256_kernelILb0EE", co)
    assert b"mlp256_swizzle_kernel" in co
    # width 128: one kernel (it picks its requant form at run time), no swizzle kernel (it reads the caller's row-major weights)
    assert re.search(rb"_Z\d+mlp128_kernel7MlpArgs", co)
    assert b"mlp128_swizzle_kernel" not in co


def test_version_108():
    hdr = open(os.path.join(ROOT, "include", "ivit.h")).read()
    assert int(re.search(r"#define IVIT_VERSION (\d+)", hdr).group(1)) >= 108
    assert _lib.load().ivit_version() >= 108
    # additions are comments only: the fused-Mlp prototypes are the ones version 107 had
    assert re.search(r"int\s+ivit_mlp_plan_create\s*\(\s*ivit_handle\s+h\s*,\s*ivit_linear_plan\s+fc1\s*,\s*ivit_linear_plan\s+fc2\s*,\s*"
                     r"ivit_mlp_plan\s*\*\s*out\s*\)", hdr)
    assert re.search(r"int\s+ivit_mlp_fused\s*\(\s*ivit_handle\s+h\s*,\s*const\s+int8_t\s*\*\s*x\s*,", hdr)
