"""Class-token attention maps without a GPU: `attention_reference` gives the reference's own recordings of blocks.i.attn.int_softmax
row 0 (and the oracle's capture where nothing is recorded), `attention_map_reference` is exact per head and one rounding in the mean,
include/ivit_attnmap.h declares four entries under version 1 beside three unchanged headers, and both kernels are in the gfx950 code
object without scratch."""
import ctypes
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden, golden_scales
import ivit_amd as iv
from ivit_amd import _abi, _lib

ENTRIES = {"ivit_attention_cls_probs": 10, "ivit_attention_map_f32": 7, "ivit_vit_attention": 12, "ivit_vit_attention_graph_create": 13}


def _oracle(g):
    from oracle import oracle as orc
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    return cfg, orc.OracleViT(cfg, iv.make_vit_weights(cfg, int(g["seed"])), golden_scales(g))


def _qk(qact1, cfg):
    """the site attn.qact1 [B, N, 3 D] -> q, k int8 [B * H, N, dh], as vit_quant.py:63-69 cuts them"""
    B, N, H, dh = qact1.shape[0], cfg.num_tokens, cfg.num_heads, cfg.head_dim
    qkv = qact1.astype(np.int8).reshape(B, N, 3, H, dh).transpose(2, 0, 3, 1, 4)
    return (np.ascontiguousarray(qkv[i]).reshape(B * H, N, dh) for i in (0, 1))


# ---------------------------------------------------------------- attention_reference against the reference's recordings
@pytest.mark.parametrize("name", ["micro_vit_b2.npz", "micro_vit2h_b3.npz"])
def test_attention_reference_equals_the_recorded_site(name):
    from ivit_amd.predict import attention_reference
    g = load_golden(name)
    cfg, o = _oracle(g)
    B, N, H = int(g["batch"]), cfg.num_tokens, cfg.num_heads
    for i in range(cfg.depth):
        p = f"blocks.{i}.attn."
        q, k = _qk(g["site/" + p + "qact1"], cfg)
        got = attention_reference(q, k, o.blocks[i]["dy_qk"], g["scale/" + p + "qact_attn1"])
        want = g["site/" + p + "int_softmax"]
        assert want.dtype == np.uint16 and want.shape == (B, H, N, N)
        assert got.dtype == np.uint16 and got.shape == (B * H, N)
        assert np.array_equal(got.reshape(B, H, N), want[:, :, 0, :]), (name, i)
        # of q only row 0 is read; the multiplier as a plain (m, r) pair is the same statement
        q2 = q.copy()
        q2[:, 1:] = 77
        dy = o.blocks[i]["dy_qk"]
        assert np.array_equal(attention_reference(q2, k, (dy[0].m, dy[0].r), g["scale/" + p + "qact_attn1"]), got)


def test_attention_reference_equals_the_oracle_capture_deit_tiny():
    from ivit_amd.predict import attention_reference
    g = load_golden("deit_tiny_b1.npz")
    cfg, o = _oracle(g)
    imgs = iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"]))
    cap = {}
    logits, _ = o.forward(imgs, capture=cap)
    assert np.array_equal(logits, g["logits_int"])
    B, N, H = imgs.shape[0], cfg.num_tokens, cfg.num_heads
    assert (N, H) == (197, 3)
    for i in range(cfg.depth):
        p = f"blocks.{i}.attn."
        q, k = _qk(cap[p + "qact1"], cfg)
        got = attention_reference(q, k, o.blocks[i]["dy_qk"], o.s[p + "qact_attn1"])
        assert np.array_equal(got.reshape(B, H, N), cap[p + "int_softmax"][:, :, 0, :]), i


def test_row_sum_of_the_numpy_statement_is_the_oracles():
    """the float32 row sum inside attention_reference against the oracle's restatement of torch's order, at every row length up to 70,
    the lengths of the real models and the entry's longest, on values large enough for every addition to round"""
    from ivit_amd.predict import _torch_order_sum
    from oracle import oracle as orc
    rng = np.random.default_rng(3)
    for n in list(range(1, 71)) + [144, 197, 256, 512, 513, 577, 1000, 1024]:
        e = np.floor(rng.uniform(0, 3.0e6, size=(3, n))).astype(np.float32)
        got = _torch_order_sum(e)
        want = [orc.lib().ivit_ref_torch_sum_f32(orc._p(np.ascontiguousarray(row)), ctypes.c_int64(n)) for row in e]
        assert got.dtype == np.float32 and np.array_equal(got, np.array(want, np.float32)), n


def test_attention_reference_refuses_a_bad_scale():
    from ivit_amd.predict import attention_reference
    q = np.zeros((1, 3, 16), np.int8)
    for bad in (0.0, -0.5, np.nan, np.inf):
        with pytest.raises(ValueError):
            attention_reference(q, q, (1.0, 1.0), bad)
    p = attention_reference(q, q, (1.0, 1.0), 0.05)             # equal scores: equal probabilities, floor(2^15 / 3) within the floor chain
    assert p.shape == (1, 3) and len(set(p[0].tolist())) == 1 and 10900 <= int(p[0, 0]) <= 10923


# ---------------------------------------------------------------- attention_map_reference
@pytest.mark.parametrize("H", [1, 3, 12, 16])
def test_attention_map_reference_exact_per_head_one_rounding_in_the_mean(H):
    from fractions import Fraction
    from ivit_amd.predict import attention_map_reference
    rng = np.random.default_rng(H)
    T = 18
    p = rng.integers(0, 32769, size=(2, 3, H, T), dtype=np.int64).astype(np.uint16)
    edge = np.array([0, 1, 32767, 32768], np.uint16)
    p[0, 0, :, 1:5] = edge                                       # every head at each edge value
    p[0, 1, :, 1:1 + 4] = 0
    p[0, 1, 0, 1:5] = edge                                       # one head at an edge value, the others 0
    p[0, 2, :, 1:5] = 32768
    p[0, 2, H - 1, 1:5] = edge                                   # ... the others at the largest value
    heads = attention_map_reference(p, heads=True)
    assert heads.dtype == np.float32 and heads.shape == (2, 3, H, T - 1)
    assert np.array_equal(heads.astype(np.float64) * 32768.0, p[..., 1:].astype(np.float64))          # p * 2^-15, exactly
    assert np.array_equal(heads[0, 0, 0, :4], np.array([0.0, 2.0 ** -15, 32767 / 32768, 1.0], np.float32))
    mean = attention_map_reference(p)
    assert mean.dtype == np.float32 and mean.shape == (2, 3, T - 1)
    S = p[..., 1:].astype(np.int64).sum(axis=-2)
    want = (S.astype(np.float64) / np.float64(H * 32768)).astype(np.float32)
    assert np.array_equal(mean.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(mean[0, 0, :4], np.array([0.0, 2.0 ** -15, 32767 / 32768, 1.0], np.float32))  # every head equal: its own value
    # one rounding: the float32 result is the nearest to the exact rational (ties cannot occur: checked against both neighbours)
    for s_, m_ in zip(S.reshape(-1)[:200].tolist(), mean.reshape(-1)[:200]):
        exact = Fraction(s_, H * 32768)
        err = abs(Fraction(float(m_)) - exact)
        for nb in (np.nextafter(m_, np.float32(2)), np.nextafter(m_, np.float32(-1))):
            assert err <= abs(Fraction(float(nb)) - exact)
    # what a float32 division of the two float32 values gives (both are below 2^24, hence exact): the same bits
    assert np.array_equal(mean, S.astype(np.float32) / np.float32(H * 32768))
    with pytest.raises(ValueError):
        attention_map_reference(np.zeros((1, 512, 4), np.uint16))


# ---------------------------------------------------------------- the fourth header and its binding
def test_attnmap_header_declares_entries_and_constants():
    hdr = open(os.path.join(ROOT, "include", "ivit_attnmap.h")).read()
    assert re.search(r'#include "ivit\.h"', hdr) and "vit_quant.py:76" in hdr and "quant_modules.py:483-497" in hdr
    assert int(re.search(r"#define IVIT_ATTNMAP_VERSION (\d+)", hdr).group(1)) == 1 == _lib.IVIT_ATTNMAP_VERSION
    assert _abi.ATTNMAP_ABI.constants == {"IVIT_ATTNMAP_VERSION": 1, "IVIT_ATTNMAP_HEADS": 0, "IVIT_ATTNMAP_MEAN": 1}
    assert (_lib.IVIT_ATTNMAP_HEADS, _lib.IVIT_ATTNMAP_MEAN) == (0, 1)
    assert list(_abi.ATTNMAP_ABI.functions) == list(ENTRIES)
    # an "Alignment:" and an "Overlap:" line in front of every entry, and the reference lines it replaces in the header
    for name in ENTRIES:
        m = re.search(r"\bint %s\(" % name, hdr)
        front = hdr[hdr.rfind(";", 0, m.start()) + 1:m.start()]
        assert len(re.findall(r"\bAlignment:", front)) == 1 and len(re.findall(r"\bOverlap:", front)) == 1, name
    assert re.search(r"int\s+ivit_attention_cls_probs\s*\(\s*ivit_handle\s+h\s*,\s*const\s+int8_t\s*\*\s*q\s*,\s*const\s+int8_t\s*\*\s*k\s*,"
                     r"\s*ivit_dyadic\s+dy_qk\s*,\s*float\s+s_softmax\s*,\s*uint16_t\s*\*\s*p_cls\s*,\s*int\s+B\s*,\s*int\s+H\s*,\s*int\s+T\s*,"
                     r"\s*int\s+dh\s*\)", hdr)
    assert re.search(r"int\s+ivit_attention_map_f32\s*\(\s*ivit_handle\s+h\s*,\s*const\s+uint16_t\s*\*\s*p_cls\s*,\s*int64_t\s+rows\s*,"
                     r"\s*int\s+H\s*,\s*int\s+T\s*,\s*int\s+mode\s*,\s*float\s*\*\s*out\s*\)", hdr)
    tail = (r"ivit_vit\s+m\s*,\s*const\s+int8_t\s*\*\s*images\s*,\s*int\s+batch\s*,\s*int\s+nslices\s*,\s*void\s*\*\s*workspace\s*,"
            r"\s*size_t\s+bytes\s*,\s*int32_t\s*\*\s*logits\s*,\s*const\s+int\s*\*\s*blocks_host\s*,\s*int\s+nblocks\s*,"
            r"\s*uint16_t\s*\*\s*attn16\s*,\s*int\s+mode\s*,\s*float\s*\*\s*map32")
    assert re.search(rf"int\s+ivit_vit_attention\s*\(\s*{tail}\s*\)", hdr)
    assert re.search(rf"int\s+ivit_vit_attention_graph_create\s*\(\s*{tail}\s*,\s*ivit_graph\s*\*\s*out\s*\)", hdr)
    assert "swin" not in "".join(ENTRIES) and re.search(r"Swin \(no class token", hdr)


# the three older headers: prototype count and sha256 of their prototypes (names, parameter types and names, in order).  Comments may
# change; what a caller compiles against may not
OLDER_HEADERS = {"ivit.h": (99, "6817c4e822691347e82f51942395393d315550b28b44df8fd32f8d739abd6b52"),
                 "ivit_eval.h": (5, "b47eee22a4d967fa3efca30b6994987eecccbe61cf040a3608941660bf3bee07"),
                 "ivit_features.h": (5, "cb523d76e256d935c2b277e969372ad9fbcde8cbdb97559fa7d84a6516f2159f")}


def _prototypes_digest(abi):
    text = "\n".join(name + "(" + ", ".join(re.sub(r"\s+", " ", d.type) + " " + d.name for d in f.params) + ")"
                     for name, f in abi.functions.items())
    return hashlib.sha256(text.encode()).hexdigest()


def test_attnmap_entries_bound_and_exported_beside_unchanged_headers():
    iv.build()
    lib = _lib.load()
    P, I, F = _lib._P, _lib._I, ctypes.c_float
    assert list(_lib.ATTNMAP_SIGNATURES) == list(ENTRIES) == list(_lib.ATTNMAP_RESTYPES)
    for name, nparams in ENTRIES.items():             # every bound name is declared, with the header's parameter count
        bound = getattr(lib, name)
        assert len(_lib.ATTNMAP_SIGNATURES[name]) == nparams and bound.argtypes == _lib.ATTNMAP_SIGNATURES[name] and bound.restype is I, name
    assert _lib.ATTNMAP_SIGNATURES["ivit_attention_cls_probs"] == [P, P, P, _lib.Dyadic, F, P, I, I, I, I]
    assert _lib.ATTNMAP_SIGNATURES["ivit_attention_map_f32"] == [P, P, ctypes.c_int64, I, I, I, P]
    assert _lib.ATTNMAP_SIGNATURES["ivit_vit_attention"] == [P, P, I, I, P, ctypes.c_size_t, P, P, I, P, I, P]
    assert _lib.ATTNMAP_SIGNATURES["ivit_vit_attention_graph_create"] == _lib.ATTNMAP_SIGNATURES["ivit_vit_attention"] + [P]
    # the three older headers: versions, prototype counts and bytes
    assert len(_lib.ABI.functions) == 99 and _lib.IVIT_VERSION == 111
    assert len(_lib.EVAL_ABI.functions) == 5 and _lib.IVIT_EVAL_VERSION == 1
    assert len(_lib.FEATURES_ABI.functions) == 5 and _lib.IVIT_FEATURES_VERSION == 1
    older = set(_lib.SIGNATURES) | set(_lib.EVAL_SIGNATURES) | set(_lib.FEATURES_SIGNATURES)
    assert not set(ENTRIES) & older
    for (name, (count, digest)), abi in zip(OLDER_HEADERS.items(), (_lib.ABI, _lib.EVAL_ABI, _lib.FEATURES_ABI)):
        assert len(abi.functions) == count and _prototypes_digest(abi) == digest, name
        text = open(os.path.join(ROOT, "include", name)).read()
        assert _prototypes_digest(_abi.parse(text) if name == "ivit.h" else _abi.parse(text, base=_lib.ABI)) == digest, name
        assert "attnmap" not in text and "_attention_cls" not in text and "ivit_vit_attention(" not in text
    with pytest.raises(_abi.AbiError):                    # it names handles of ivit.h: it parses only with ivit.h as its base
        _abi.parse(open(_abi.ATTNMAP_HEADER).read())


def test_build_follows_the_attnmap_header():
    so = iv.build()
    assert os.path.getmtime(so) >= os.path.getmtime(_abi.ATTNMAP_HEADER)
    assert "ivit_attnmap.h" in _lib.SOURCES
    src = open(os.path.join(ROOT, "i-vit_amd", "_lib.py")).read()
    assert re.search(r"newest = max\(.*_abi\.FEATURES_HEADER.*_abi\.ATTNMAP_HEADER", src)


def test_swin_engine_has_no_attention():
    from ivit_amd.engine import ViTEngine
    from ivit_amd.swin_engine import SwinEngine
    assert hasattr(ViTEngine, "attention") and hasattr(ViTEngine, "capture_attention")
    assert not hasattr(SwinEngine, "attention") and not hasattr(SwinEngine, "capture_attention")
    assert not any("swin" in n for n in _lib.ATTNMAP_SIGNATURES)


def test_attention_blocks_normalisation():
    """the block list of ViTEngine.attention, judged on the host before anything else (no device needed for the rule itself)"""
    from types import SimpleNamespace
    from ivit_amd.engine import ViTEngine
    norm = lambda blocks: ViTEngine._attention_blocks(SimpleNamespace(cfg=SimpleNamespace(depth=12)), blocks)
    assert norm(-1) == (11,) and norm(0) == (0,) and norm((0, 5, 11)) == (0, 5, 11) and norm([0, -1]) == (0, 11)
    assert norm((-12, -1)) == (0, 11) and norm(np.int64(3)) == (3,)
    for bad in ((), (1, 1), (5, 0), (0, -12), (-1, 0), 12, -13, (0, 12), (0.5,), ("1",)):
        with pytest.raises(ValueError):
            norm(bad)


# ---------------------------------------------------------------- the kernels in the code object
def test_attnmap_kernels_in_code_object_without_scratch(tmp_path):
    from test_cabi_cpu import _device_code_object
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
        spill = re.search(r"\.vgpr_spill_count:\s+(\d+)", blk)
        if nm and scratch and spill:
            kernels[nm.group(1)] = (int(scratch.group(1)), int(spill.group(1)))
    assert len(kernels) > 100, "code object metadata looks wrong"
    want = [k for k in kernels if re.fullmatch(r"_Z\d+attn_cls_probs_kernel\w+", k)]
    want += [k for k in kernels if re.fullmatch(r"_Z\d+attn_map_f32_kernelILb[01]EE\w+", k)]
    assert len(want) == 3, want                      # the tap, and the map's two modes
    for k in want:
        assert kernels[k] == (0, 0), (k, kernels[k])
