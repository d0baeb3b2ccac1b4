"""The last ViT block's tail on the class-token rows only (csrc/ivit_model.h, cls_tail): the premise on the CPU oracle's operators, the
class-token instantiations of the fused attention in the gfx950 code object, and the C ABI's additions (version 109)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden, golden_scales
import ivit_amd as iv
from ivit_amd import _lib
from test_cabi_cpu import _device_code_object


def _cls_forward(o, images):
    """OracleViT.forward with the last block's attention, proj, norm2 and Mlp on row 0 of each image: q, the identity branch and
    everything behind the attention for that row alone, k and v of all rows.  The blocks before and the last block's norm1 + qkv
    come from a full forward's captures (they are the same computation)."""
    from oracle import oracle as orc
    cfg, c, s = o.cfg, o.c, o.s
    B = images.shape[0]
    N, D, H, dh = cfg.num_tokens, cfg.embed_dim, cfg.num_heads, cfg.head_dim
    cap = {}
    full, _ = o.forward(images, capture=cap)
    i = cfg.depth - 1
    p, b = f"blocks.{i}.", o.blocks[i]
    x_in = cap[f"blocks.{i - 1}.qact4"] if i else cap["qact1"]                  # [B, N, D], the last block's input
    qkv = cap[p + "attn.qact1"].astype(np.int8).reshape(B, N, 3, H, dh).transpose(2, 0, 3, 1, 4)
    q0 = np.ascontiguousarray(qkv[0][:, :, :1, :]).reshape(B * H, 1, dh)         # the class token's query, per head
    k = qkv[1].reshape(B * H, N, dh)
    v = qkv[2].reshape(B * H, N, dh)
    sc8 = orc.requant(orc.bmm_nt_i8(q0, k), b["dy_qk"], 8)                       # [B*H, 1, N]
    pr = orc.shiftmax(sc8.astype(np.int8), s[p + "attn.qact_attn1"], 16)
    ctx = orc.bmm_av(pr, v).reshape(B, H * dh)                                   # heads merged: row b, columns 64 h ...
    ctx8 = orc.requant(ctx, b["dy_av"], 8)
    y = orc.requant(orc.linear_i8(ctx8.astype(np.int8), b["proj"][0], b["proj"][1]), b["proj"][2], 16)
    x = orc.requant(y, b["dy_res1"][0], 16, np.ascontiguousarray(x_in[:, 0, :]), b["dy_res1"][1])     # [B, D]
    a = orc.requant(orc.layernorm(x.astype(np.int16), s[p + "qact2"], *b["ln2"]), b["dy_ln2"], 8)
    h = orc.requant(orc.linear_i8(a.astype(np.int8), b["fc1"][0], b["fc1"][1]), b["fc1"][2], 8)
    g8 = orc.requant(orc.shiftgelu(h.astype(np.int8), s[p + "mlp.qact_gelu"]).astype(np.int32), b["dy_gelu"], 8)
    y = orc.requant(orc.linear_i8(g8.astype(np.int8), b["fc2"][0], b["fc2"][1]), b["fc2"][2], 16)
    x = orc.requant(y, b["dy_res2"][0], 16, x, b["dy_res2"][1])
    assert np.array_equal(x, cap[p + "qact4"][:, 0, :]), "class-token rows of the residual stream differ"
    a = orc.requant(orc.layernorm(x.astype(np.int16), s[p + "qact4"], *c["ln"]), c["dy_ln"], 8)
    return full, orc.linear_i8(a.astype(np.int8), c["head"][0], c["head"][1])


@pytest.mark.parametrize("name", ["micro_vit_b2.npz", "micro_vit2h_b3.npz", "deit_tiny_b1.npz"])
def test_logits_need_only_the_class_token_rows_of_the_last_block(name):
    from oracle import oracle as orc
    g = load_golden(name)
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    o = orc.OracleViT(cfg, iv.make_vit_weights(cfg, int(g["seed"])), golden_scales(g))
    imgs = iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"]))
    full, cls = _cls_forward(o, imgs)
    assert np.array_equal(full, g["logits_int"])
    assert np.array_equal(cls, full)


def test_cls_attention_kernels_in_code_object(tmp_path):
    """Every class-token instantiation (template <NB, FAST, TT, LUT, VROW, CLS = true> of attn_fused_kernel: three key-block counts
    times row table with v row-major / v^T, two-level tables, arithmetic fast / exact) and the row gather are in the gfx950 code
    object and use no scratch."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        readelf = shutil.which("llvm-readelf")
    assert readelf, "llvm-readelf not found"
    co = tmp_path / "dev.co"
    co.write_bytes(_device_code_object(iv.build()))
    notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True, check=True).stdout
    kernels = {}
    for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        scratch = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if nm and scratch:
            kernels[nm.group(1)] = int(scratch.group(1))
    assert len(kernels) > 100, "code object metadata looks wrong"
    want = [f"_Z17attn_fused_kernelILi{nb}ELb{fast}ELi0ELi{lut}ELb{vrow}ELb1EEv8AttnArgs"
            for nb in (1, 4, 10) for fast, lut, vrow in ((1, 2, 1), (1, 2, 0), (1, 1, 0), (1, 0, 0), (0, 0, 0))]
    want.append("_Z20gather_rows16_kernelPKsxixPs")
    for k in want:
        assert k in kernels, k
        assert kernels[k] == 0, (k, kernels[k])


def test_header_and_bindings():
    hdr = open(os.path.join(ROOT, "include", "ivit.h")).read()
    assert int(re.search(r"#define IVIT_VERSION (\d+)", hdr).group(1)) >= 109
    tail = r"int8_t\s*\*\s*ctx_cls\s*,\s*const\s+int16_t\s*\*\s*x16\s*,\s*int16_t\s*\*\s*x_cls\s*,\s*int\s+B\s*,\s*int\s+H\s*,\s*int\s+T\s*,\s*int\s+dh\s*,\s*int\s+ldv\s*\)"
    for name in ("ivit_attention_fused_cls", "ivit_attention_fused_lut_cls", "ivit_attention_fused_rowlut_cls"):
        assert re.search(r"int\s+" + name + r"\s*\(\s*ivit_handle\s+h\s*,[^)]*" + tail, hdr), name
    assert re.search(r"int\s+ivit_gather_rows_i16\s*\(\s*ivit_handle\s+h\s*,\s*const\s+int16_t\s*\*\s*x\s*,\s*int64_t\s+rows\s*,\s*int\s+C\s*,"
                     r"\s*int64_t\s+row_stride\s*,\s*int16_t\s*\*\s*out\s*\)", hdr)
    assert re.search(r"int\s+ivit_vit_cls_tail\s*\(\s*ivit_vit\s+m\s*,\s*int\s+batch\s*,\s*int\s*\*\s*on\s*\)", hdr)
    iv.build()
    lib = _lib.load()
    assert lib.ivit_version() >= 109
    for name in ("ivit_attention_fused_cls", "ivit_attention_fused_lut_cls", "ivit_attention_fused_rowlut_cls", "ivit_gather_rows_i16",
                 "ivit_vit_cls_tail"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
