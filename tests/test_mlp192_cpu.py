"""The width-192 fused Mlp exists in the built library without a GPU to run it: its kernel is in the gfx950 code object, and
the public header declares the two queries that report what the runners launch."""
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


def test_mlp192_kernel_compiled_for_gfx950():
    co = _device_code_object(iv.build())
    assert b"mlp192_kernel" in co and b"mlp192_swizzle_kernel" in co
    # both requant forms of the kernel (single-FMA and multiply-add) are instantiated
    assert re.search(rb"_Z\d+mlp192_kernelILb1EE", co) and re.search(rb"_Z\d+mlp192_kernelILb0EE", co)


def test_header_declares_fused_mlp_queries():
    hdr = open(os.path.join(ROOT, "include", "ivit.h")).read()
    assert re.search(r"int\s+ivit_vit_fused_mlp_blocks\s*\(\s*ivit_vit\s+m\s*,\s*int\s+batch\s*,\s*int\s*\*\s*blocks\s*\)", hdr)
    assert re.search(r"int\s+ivit_swin_fused_mlp_blocks\s*\(\s*ivit_swin\s+m\s*,\s*int\s+batch\s*,\s*int\s+blocks_per_stage\[4\]\s*\)", hdr)
    assert int(re.search(r"#define IVIT_VERSION (\d+)", hdr).group(1)) >= 107
    lib = _lib.load()
    for name in ("ivit_vit_fused_mlp_blocks", "ivit_swin_fused_mlp_blocks"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.ivit_version() >= 107
