"""norm2 inside the lock-step fused Mlp launch (ivit_layernorm_mlp_lockstep_planned; mlp192ln_kernel / mlp384ln_kernel of
csrc/ivit_mlp.h) exists in the public interface and in the built library without a GPU to run it."""
import os
import re

import ivit_amd as iv
from ivit_amd import _lib
from test_mlp192_cpu import _device_code_object

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERSION = 111


def test_header_declares_lockstep_ln_mlp():
    hdr = open(os.path.join(ROOT, "include", "ivit.h")).read()
    assert re.search(r"int\s+ivit_layernorm_mlp_lockstep_planned\s*\(\s*ivit_handle\s+h\s*,\s*ivit_mlp_plan\s+p\s*,\s*const\s+int16_t\s*\*\s*x16\s*,"
                     r"\s*float\s+scale\s*,\s*const\s+float\s*\*\s*bias_int\s*,\s*const\s+float\s*\*\s*sc\s*,\s*const\s+ivit_dyadic\s*\*\s*ln_dy\s*,"
                     r"\s*const\s+int8_t\s*\*\s*gelu_table\s*,\s*ivit_dyadic\s+dy_main\s*,\s*ivit_dyadic\s+dy_res\s*,\s*int16_t\s*\*\s*out\s*,"
                     r"\s*int64_t\s+M\s*\)", hdr)
    assert re.search(r"int\s+ivit_vit_fused_ln_mlp_blocks\s*\(\s*ivit_vit\s+m\s*,\s*int\s+batch\s*,\s*int\s*\*\s*blocks\s*\)", hdr)
    assert int(re.search(r"#define IVIT_VERSION (\d+)", hdr).group(1)) == VERSION
    # the header comment names the reference's lines the launch stands for
    assert "vit_quant.py:139-142" in hdr and "layers_quant.py:144-153" in hdr


def test_signatures_bind_both():
    assert len(_lib.SIGNATURES["ivit_layernorm_mlp_lockstep_planned"]) == 12
    assert len(_lib.SIGNATURES["ivit_vit_fused_ln_mlp_blocks"]) == 3


def test_library_exports_both():
    lib = _lib.load()
    for name in ("ivit_layernorm_mlp_lockstep_planned", "ivit_vit_fused_ln_mlp_blocks"):
        assert hasattr(lib, name), name
    assert lib.ivit_version() == VERSION


def test_lockstep_ln_kernels_compiled_for_gfx950():
    """Both widths, both requant forms of the GEMM phases; the plain kernels keep their names beside them."""
    co = _device_code_object(iv.build())
    for k in (b"mlp192ln_kernel", b"mlp384ln_kernel"):
        assert re.search(rb"_Z\d+" + k + rb"ILb1EE", co) and re.search(rb"_Z\d+" + k + rb"ILb0EE", co), k
    for k in (b"mlp192_kernel", b"mlp384_kernel"):
        assert re.search(rb"_Z\d+" + k + rb"ILb1EE", co) and re.search(rb"_Z\d+" + k + rb"ILb0EE", co), k
