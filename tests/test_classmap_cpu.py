"""Class-activation maps of a Swin without a GPU: `class_map_reference` on the reference's own recording of the final-stage tokens
(site/qact2) and the head's integers, the exact sum identity behind the maps, the out-of-range convention and the two-step fp32
expression; include/ivit_classmap.h declares three entries and three constants under version 1 beside four unchanged headers; the
binding follows it; and both instantiations of class_map_kernel are in the gfx950 code object without scratch."""
import ctypes
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
import ivit_amd as iv
from ivit_amd import _abi, _lib
from ivit_amd.predict import class_map_reference

ENTRIES = {"ivit_class_map": 12, "ivit_swin_class_map": 16, "ivit_swin_class_map_graph_create": 17}


@pytest.fixture(scope="module")
def recorded():
    """the reference's recording of one forward of the micro Swin: tokens behind qact2 [2, 49, 64], the head's integers [10, 64]"""
    g, sd = load_golden("micro_swin_b2.npz"), load_golden("micro_swin_state_dict.npz")
    assert str(g["cfg_name"]) == str(sd["cfg_name"]) and int(g["seed"]) == int(sd["seed"])
    tok = g["site/qact2"]
    assert tok.shape == (2, 49, 64) and tok.min() >= -128 and tok.max() <= 127
    w, bias = sd["buf/head.weight_integer"], sd["buf/head.bias_integer"]
    assert w.shape == (10, 64) and np.array_equal(w, np.rint(w)) and np.abs(w).max() <= 127
    # the same model: the head of the state dict applied to the recorded pooled row is the recorded head output
    q3 = g["site/qact3"].reshape(2, 64).astype(np.int64)
    assert np.array_equal(q3 @ w.astype(np.int64).T + bias.astype(np.int64), g["site/head"]) and np.array_equal(g["site/head"], g["logits_int"])
    class_scale = (np.float32(g["scale/qact2"]) * sd["buf/head.fc_scaling_factor"]).astype(np.float32)
    tok8, head_w = tok.astype(np.int8), w.astype(np.int8)
    for a in (tok8, head_w, class_scale):
        a.setflags(write=False)
    return g, tok8, head_w, class_scale


# ---------------------------------------------------------------- class_map_reference
def test_class_map_reference_on_the_recorded_tokens(recorded):
    g, tok8, head_w, class_scale = recorded
    B, L, C = tok8.shape
    idx = np.tile(np.arange(10, dtype=np.int32), (B, 1))
    cam32, map32 = class_map_reference(tok8, head_w, idx, class_scale)
    assert cam32.dtype == np.int32 and cam32.shape == (B, 10, L) and map32.dtype == np.float32 and map32.shape == (B, 10, L)
    want = np.einsum("kc,btc->bkt", head_w.astype(np.int64), tok8.astype(np.int64))
    assert np.array_equal(cam32.astype(np.int64), want) and np.abs(want).max() > 1000            # not a trivial recording
    # the identity behind the maps, exactly: the sum of a map is the weight row against the token sum
    assert np.array_equal(cam32.astype(np.int64).sum(axis=2), np.einsum("kc,bc->bk", head_w.astype(np.int64), tok8.astype(np.int64).sum(axis=1)))
    # map32 is the two-step fp32 expression: an exact conversion, one float32 multiply
    two_step = cam32.astype(np.float32) * class_scale[None, :, None]
    assert two_step.dtype == np.float32 and np.array_equal(map32.view(np.uint32), two_step.view(np.uint32))
    assert np.array_equal(cam32.astype(np.float32).astype(np.int64), cam32)
    assert np.array_equal(map32, (cam32.astype(np.float64) * class_scale.astype(np.float64)[None, :, None]).astype(np.float32))
    assert class_map_reference(tok8, head_w, idx)[1] is None and np.array_equal(class_map_reference(tok8, head_w, idx)[0], cam32)
    # any selection of classes is the selection of those rows; duplicates are allowed
    pick = np.array([[3, 3, 9], [0, 7, 0]], np.int32)
    c2, m2 = class_map_reference(tok8, head_w, pick, class_scale)
    for b in range(B):
        assert np.array_equal(c2[b], cam32[b, pick[b]]) and np.array_equal(m2[b].view(np.uint32), map32[b, pick[b]].view(np.uint32))


def test_class_map_reference_out_of_range_index(recorded):
    g, tok8, head_w, class_scale = recorded
    idx = np.array([[-1, 4, 10], [2 ** 31 - 1, -2 ** 31, 4]], np.int32)
    cam32, map32 = class_map_reference(tok8, head_w, idx, class_scale)
    full = class_map_reference(tok8, head_w, np.full((2, 1), 4, np.int32), class_scale)
    for b, j in ((0, 0), (0, 2), (1, 0), (1, 1)):
        assert not cam32[b, j].any() and np.isnan(map32[b, j]).all() and np.all(map32[b, j].view(np.uint32) == 0x7FC00000)
    for b, j in ((0, 1), (1, 2)):
        assert np.array_equal(cam32[b, j], full[0][b, 0]) and np.array_equal(map32[b, j].view(np.uint32), full[1][b, 0].view(np.uint32))


def test_class_map_reference_extreme_and_refused_widths():
    tok8 = np.full((1, 2, 1024), -128, np.int8)
    head_w = np.full((1, 1024), -127, np.int8)
    cam32, map32 = class_map_reference(tok8, head_w, np.zeros((1, 1), np.int32), np.ones(1, np.float32))
    assert np.all(cam32 == 16646144) and 16646144 < 2 ** 24 and np.all(map32 == np.float32(16646144.0))
    for C in (24, 1040):
        with pytest.raises(ValueError):
            class_map_reference(np.zeros((1, 2, C), np.int8), np.zeros((3, C), np.int8), np.zeros((1, 1), np.int32))


# ---------------------------------------------------------------- the fifth header and its binding
def test_classmap_header_declares_entries_and_constants():
    hdr = open(os.path.join(ROOT, "include", "ivit_classmap.h")).read()
    assert re.search(r'#include "ivit\.h"', hdr) and "swin_quant.py:551-564" in hdr and "quant_modules.py:67-97" in hdr
    assert int(re.search(r"#define IVIT_CLASSMAP_VERSION (\d+)", hdr).group(1)) == 1 == _lib.IVIT_CLASSMAP_VERSION
    assert _abi.CLASSMAP_ABI.constants == {"IVIT_CLASSMAP_VERSION": 1, "IVIT_CLASSMAP_TOPK": 0, "IVIT_CLASSMAP_GIVEN": 1}
    assert (_lib.IVIT_CLASSMAP_TOPK, _lib.IVIT_CLASSMAP_GIVEN) == (0, 1)
    assert list(_abi.CLASSMAP_ABI.functions) == list(ENTRIES)
    for name in ENTRIES:                                  # one "Alignment:" and one "Overlap:" line in front of every entry
        m = re.search(r"\bint %s\(" % name, hdr)
        front = hdr[hdr.rfind(";", 0, m.start()) + 1:m.start()]
        assert len(re.findall(r"\bAlignment:", front)) == 1 and len(re.findall(r"\bOverlap:", front)) == 1, name
    assert re.search(r"int\s+ivit_class_map\s*\(\s*ivit_handle\s+h\s*,\s*const\s+int8_t\s*\*\s*tok8\s*,\s*const\s+int8_t\s*\*\s*head_w\s*,"
                     r"\s*const\s+int32_t\s*\*\s*idx\s*,\s*int\s+batch\s*,\s*int\s+L\s*,\s*int\s+C\s*,\s*int\s+num_classes\s*,\s*int\s+k\s*,"
                     r"\s*const\s+float\s*\*\s*class_scale\s*,\s*int32_t\s*\*\s*cam32\s*,\s*float\s*\*\s*map32\s*\)", hdr)
    tail = (r"ivit_swin\s+m\s*,\s*const\s+int8_t\s*\*\s*images\s*,\s*int\s+batch\s*,\s*int\s+nslices\s*,\s*void\s*\*\s*workspace\s*,"
            r"\s*size_t\s+bytes\s*,\s*int32_t\s*\*\s*logits\s*,\s*const\s+float\s*\*\s*head_scale\s*,\s*int\s+mode\s*,\s*int\s+k\s*,"
            r"\s*int32_t\s*\*\s*idx\s*,\s*float\s*\*\s*val\s*,\s*int8_t\s*\*\s*tok8\s*,\s*const\s+float\s*\*\s*class_scale\s*,"
            r"\s*int32_t\s*\*\s*cam32\s*,\s*float\s*\*\s*map32")
    assert re.search(rf"int\s+ivit_swin_class_map\s*\(\s*{tail}\s*\)", hdr)
    assert re.search(rf"int\s+ivit_swin_class_map_graph_create\s*\(\s*{tail}\s*,\s*ivit_graph\s*\*\s*out\s*\)", hdr)
    assert "vit" not in "".join(ENTRIES).replace("ivit", "")


# the four older headers: prototype count and sha256 of their prototypes (names, parameter types and names, in order).  The first
# three digests are those test_attnmap_cpu.py pins; ivit_attnmap.h's was computed with the same function on the parent commit
OLDER_HEADERS = {"ivit.h": (99, 111, "6817c4e822691347e82f51942395393d315550b28b44df8fd32f8d739abd6b52"),
                 "ivit_eval.h": (5, 1, "b47eee22a4d967fa3efca30b6994987eecccbe61cf040a3608941660bf3bee07"),
                 "ivit_features.h": (5, 1, "cb523d76e256d935c2b277e969372ad9fbcde8cbdb97559fa7d84a6516f2159f"),
                 "ivit_attnmap.h": (4, 1, "2f429e1f49a79e9a910707d666d5d274831c1f49f0e8177fd51abf43952572f6")}


def _prototypes_digest(abi):
    text = "\n".join(name + "(" + ", ".join(re.sub(r"\s+", " ", d.type) + " " + d.name for d in f.params) + ")"
                     for name, f in abi.functions.items())
    return hashlib.sha256(text.encode()).hexdigest()


def test_classmap_entries_bound_and_exported_beside_unchanged_headers():
    iv.build()
    lib = _lib.load()
    P, I = _lib._P, _lib._I
    assert list(_lib.CLASSMAP_SIGNATURES) == list(ENTRIES) == list(_lib.CLASSMAP_RESTYPES)
    for name, nparams in ENTRIES.items():             # every bound name is declared, with the header's parameter count
        bound = getattr(lib, name)
        assert len(_lib.CLASSMAP_SIGNATURES[name]) == nparams and bound.argtypes == _lib.CLASSMAP_SIGNATURES[name] and bound.restype is I, name
    assert _lib.CLASSMAP_SIGNATURES["ivit_class_map"] == [P, P, P, P, I, I, I, I, I, P, P, P]
    assert _lib.CLASSMAP_SIGNATURES["ivit_swin_class_map"] == [P, P, I, I, P, ctypes.c_size_t, P, P, I, I, P, P, P, P, P, P]
    assert _lib.CLASSMAP_SIGNATURES["ivit_swin_class_map_graph_create"] == _lib.CLASSMAP_SIGNATURES["ivit_swin_class_map"] + [P]
    versions = (_lib.IVIT_VERSION, _lib.IVIT_EVAL_VERSION, _lib.IVIT_FEATURES_VERSION, _lib.IVIT_ATTNMAP_VERSION)
    abis = (_lib.ABI, _lib.EVAL_ABI, _lib.FEATURES_ABI, _lib.ATTNMAP_ABI)
    older = set()
    for (name, (count, version, digest)), abi, v in zip(OLDER_HEADERS.items(), abis, versions):
        assert len(abi.functions) == count and v == version and _prototypes_digest(abi) == digest, name
        text = open(os.path.join(ROOT, "include", name)).read()
        assert _prototypes_digest(_abi.parse(text) if name == "ivit.h" else _abi.parse(text, base=_lib.ABI)) == digest, name
        assert "classmap" not in text and "class_map" not in text, name
        older |= set(abi.functions)
    assert not set(ENTRIES) & older
    with pytest.raises(_abi.AbiError):                    # it names handles of ivit.h: it parses only with ivit.h as its base
        _abi.parse(open(_abi.CLASSMAP_HEADER).read())


def test_build_follows_the_classmap_header():
    so = iv.build()
    assert os.path.getmtime(so) >= os.path.getmtime(_abi.CLASSMAP_HEADER)
    assert "ivit_classmap.h" in _lib.SOURCES and os.path.exists(os.path.join(ROOT, "i-vit_amd", "csrc", "ivit_classmap.h"))
    src = open(os.path.join(ROOT, "i-vit_amd", "_lib.py")).read()
    assert re.search(r"newest = max\(.*_abi\.ATTNMAP_HEADER, _abi\.CLASSMAP_HEADER", src)


def test_class_map_is_a_swin_feature_and_attention_a_vit_one():
    from ivit_amd.engine import ViTEngine
    from ivit_amd.swin_engine import SwinEngine
    assert hasattr(SwinEngine, "class_map") and hasattr(SwinEngine, "capture_class_map")
    assert hasattr(SwinEngine, "token_scale_host") and hasattr(SwinEngine, "class_scale")
    assert not hasattr(ViTEngine, "class_map") and not hasattr(ViTEngine, "capture_class_map")
    assert not hasattr(SwinEngine, "attention") and not hasattr(SwinEngine, "capture_attention")
    assert not any(n.startswith("ivit_vit_") for n in _lib.CLASSMAP_SIGNATURES)


# ---------------------------------------------------------------- the kernel in the code object
def test_classmap_kernels_in_code_object_without_scratch(tmp_path):
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
    want = sorted(k for k in kernels if re.fullmatch(r"_Z\d+class_map_kernelILb[01]EE\w+", k))
    assert len(want) == 2 and "ILb0E" in want[0] and "ILb1E" in want[1], want       # without and with map32
    for k in want:
        assert kernels[k] == (0, 0), (k, kernels[k])
