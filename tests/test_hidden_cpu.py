"""Hidden states without a GPU: `hidden_reference` on hand-worked cases (both ends of int16, zero, the reference's smallest scale and
one above 1) and on the reference's own recordings of a block's output; its grid form is the transpose of its tokens form;
include/ivit_hidden.h declares seven entries and three constants under version 1 beside five unchanged headers; the binding follows
it; the build follows its mtime; and both instantiations of hidden_f32_kernel are in the gfx950 code object without scratch."""
import ctypes
import hashlib
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
import ivit_amd as iv
from ivit_amd import _abi, _lib
from ivit_amd.predict import hidden_reference

ENTRIES = {"ivit_hidden_f32": 9, "ivit_vit_hidden_scale": 3, "ivit_swin_hidden_scale": 3, "ivit_vit_hidden_states": 12,
           "ivit_vit_hidden_states_graph_create": 13, "ivit_swin_hidden_states": 12, "ivit_swin_hidden_states_graph_create": 13}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- hidden_reference
def test_hidden_reference_hand_worked_cases():
    q = np.array([[[-32768, 32767, 0, 1, -1, 3, 12345, -12345]]], np.int16)
    # 2^-23, the floor of the reference's scales: every product is the integer with the exponent moved, exact
    out = hidden_reference(q, np.float32(2.0 ** -23))
    assert out.dtype == np.float32 and out.shape == (1, 1, 8)
    want = [struct.unpack("<I", struct.pack("<f", v))[0] for v in
            (-2.0 ** -8, 32767 * 2.0 ** -23, 0.0, 2.0 ** -23, -2.0 ** -23, 3 * 2.0 ** -23, 12345 * 2.0 ** -23, -12345 * 2.0 ** -23)]
    assert bits(out).reshape(-1).tolist() == want
    assert bits(out)[0, 0, 0] == 0xBB800000 and bits(out)[0, 0, 1] == 0x3B7FFE00 and bits(out)[0, 0, 2] == 0
    # a scale above 1 that is no power of two: one rounding of the exact product, worked in float64 (53 bits hold 16 x 24 exactly)
    s = np.float32(1.7)
    out = hidden_reference(q, s)
    exact = (q.astype(np.float64) * np.float64(s)).astype(np.float32)
    assert np.array_equal(bits(out), bits(exact))
    assert out[0, 0, 0] == np.float32(-32768.0) * s and out[0, 0, 1] == np.float32(32767.0) * s and bits(out)[0, 0, 2] == 0
    assert bits(out)[0, 0, 0] == 0xC759999A                # -32768 * fl32(1.7): 0x3FD9999A with 15 added to its exponent, and the sign
    # a scale of exactly 1 returns the integers
    assert np.array_equal(hidden_reference(q, 1.0), q.astype(np.float32))
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            hidden_reference(q, bad)
    with pytest.raises(ValueError):
        hidden_reference(np.zeros((1, 2, 12), np.int16), 1.0)
    with pytest.raises(ValueError):
        hidden_reference(q, 1.0, t0=1)                        # T = 1: no row is left
    with pytest.raises(ValueError):
        hidden_reference(q, 1.0, layout="nchw")


@pytest.mark.parametrize("t0", [0, 1])
def test_hidden_reference_grid_is_the_transpose_of_tokens(t0):
    rng = np.random.default_rng(3 + t0)
    q = rng.integers(-32768, 32768, size=(3, 17, 24), dtype=np.int64).astype(np.int16)
    q[0, t0, 0], q[2, 16, 23] = -32768, 32767
    s = np.float32(0.0123)
    tok, grid = hidden_reference(q, s, "tokens", t0), hidden_reference(q, s, "grid", t0)
    assert tok.shape == (3, 17 - t0, 24) and grid.shape == (3, 24, 17 - t0) and grid.flags["C_CONTIGUOUS"]
    assert np.array_equal(bits(grid), bits(tok.transpose(0, 2, 1)))
    assert np.array_equal(bits(tok), bits(hidden_reference(q, s, "tokens", 0)[:, t0:]))       # the first t0 rows dropped, nothing else


@pytest.mark.parametrize("fname,keys", [("micro_vit_b2.npz", ["blocks.0.qact4", "blocks.1.qact4"]),
                                        ("micro_vit2h_b3.npz", ["blocks.0.qact4", "blocks.1.qact4"]),
                                        ("micro_swin_b2.npz", ["layers.0.blocks.1.qact4", "layers.1.blocks.1.qact4"])])
def test_hidden_reference_on_the_recorded_sites(fname, keys):
    """the reference's recording of the site: integers that fit int16 (both ends reached in the micro ViTs) and a scale; the fp32
    form is q * s in one multiply, as QuantAct.forward returns it"""
    g = load_golden(fname)
    lo, hi = 0, 0
    for k in keys:
        site, s = g["site/" + k], np.float32(g["scale/" + k])
        assert site.ndim == 3 and site.min() >= -32768 and site.max() <= 32767 and s > 0
        lo, hi = min(lo, int(site.min())), max(hi, int(site.max()))
        out = hidden_reference(site.astype(np.int16), s)
        assert np.array_equal(bits(out), bits(site.astype(np.float32) * s))
        assert np.array_equal(out, (site.astype(np.float64) * np.float64(s)).astype(np.float32))
    if "vit" in fname:
        assert (lo, hi) == (-32768, 32767), "the saturated ends are in the pin"


# ---------------------------------------------------------------- the sixth header and its binding
def test_hidden_header_declares_entries_and_constants():
    hdr = open(os.path.join(ROOT, "include", "ivit_hidden.h")).read()
    assert re.search(r'#include "ivit\.h"', hdr)
    for cite in ("vit_quant.py:130-143", "swin_quant.py", "SwinTransformerBlock.forward", "BasicLayer.forward", "quant_modules.py:204-206"):
        assert cite in hdr, cite
    assert int(re.search(r"#define IVIT_HIDDEN_VERSION (\d+)", hdr).group(1)) == 1 == _lib.IVIT_HIDDEN_VERSION
    assert _abi.HIDDEN_ABI.constants == {"IVIT_HIDDEN_VERSION": 1, "IVIT_HIDDEN_TOKENS": 0, "IVIT_HIDDEN_GRID": 1}
    assert (_lib.IVIT_HIDDEN_TOKENS, _lib.IVIT_HIDDEN_GRID) == (0, 1)
    assert list(_abi.HIDDEN_ABI.functions) == list(ENTRIES)
    for name in ENTRIES:                                  # one "Alignment:" and one "Overlap:" line in front of every entry
        m = re.search(r"\bint %s\(" % name, hdr)
        front = hdr[hdr.rfind(";", 0, m.start()) + 1:m.start()]
        assert len(re.findall(r"\bAlignment:", front)) == 1 and len(re.findall(r"\bOverlap:", front)) == 1, name
    assert re.search(r"int\s+ivit_hidden_f32\s*\(\s*ivit_handle\s+h\s*,\s*const\s+int16_t\s*\*\s*x16\s*,\s*float\s+scale\s*,\s*int\s+batch\s*,"
                     r"\s*int\s+T\s*,\s*int\s+C\s*,\s*int\s+t0\s*,\s*int\s+layout\s*,\s*float\s*\*\s*out\s*\)", hdr)
    for model, lst, cnt in (("vit", "blocks_host", "nblocks"), ("swin", "stages_host", "nstages")):
        tail = (rf"ivit_{model}\s+m\s*,\s*const\s+int8_t\s*\*\s*images\s*,\s*int\s+batch\s*,\s*int\s+nslices\s*,\s*void\s*\*\s*workspace\s*,"
                rf"\s*size_t\s+bytes\s*,\s*int32_t\s*\*\s*logits\s*,\s*const\s+int\s*\*\s*{lst}\s*,\s*int\s+{cnt}\s*,\s*int16_t\s*\*\s*hid16\s*,"
                r"\s*int\s+layout\s*,\s*float\s*\*\s*hid32")
        assert re.search(rf"int\s+ivit_{model}_hidden_states\s*\(\s*{tail}\s*\)", hdr), model
        assert re.search(rf"int\s+ivit_{model}_hidden_states_graph_create\s*\(\s*{tail}\s*,\s*ivit_graph\s*\*\s*out\s*\)", hdr), model
        assert re.search(rf"int\s+ivit_{model}_hidden_scale\s*\(\s*ivit_{model}\s+m\s*,\s*int\s+\w+\s*,\s*float\s*\*\s*scale_host\s*\)", hdr), model


# the five older headers: prototype count, version and sha256 of their prototypes (names, parameter types and names, in order).  The
# first four digests are those test_classmap_cpu.py pins; ivit_classmap.h's was computed with the same function on the parent commit
OLDER_HEADERS = {"ivit.h": (99, 111, "6817c4e822691347e82f51942395393d315550b28b44df8fd32f8d739abd6b52"),
                 "ivit_eval.h": (5, 1, "b47eee22a4d967fa3efca30b6994987eecccbe61cf040a3608941660bf3bee07"),
                 "ivit_features.h": (5, 1, "cb523d76e256d935c2b277e969372ad9fbcde8cbdb97559fa7d84a6516f2159f"),
                 "ivit_attnmap.h": (4, 1, "2f429e1f49a79e9a910707d666d5d274831c1f49f0e8177fd51abf43952572f6"),
                 "ivit_classmap.h": (3, 1, "8da355354133cbf09e4e986c0bb6e4081b79ba6c60ac3fdb746cceec64bc3620")}


def _prototypes_digest(abi):
    text = "\n".join(name + "(" + ", ".join(re.sub(r"\s+", " ", d.type) + " " + d.name for d in f.params) + ")"
                     for name, f in abi.functions.items())
    return hashlib.sha256(text.encode()).hexdigest()


def test_hidden_entries_bound_and_exported_beside_unchanged_headers():
    iv.build()
    lib = _lib.load()
    P, I, F = _lib._P, _lib._I, ctypes.c_float
    assert list(_lib.HIDDEN_SIGNATURES) == list(ENTRIES) == list(_lib.HIDDEN_RESTYPES)
    for name, nparams in ENTRIES.items():             # every bound name is declared, with the header's parameter count
        bound = getattr(lib, name)
        assert len(_lib.HIDDEN_SIGNATURES[name]) == nparams and bound.argtypes == _lib.HIDDEN_SIGNATURES[name] and bound.restype is I, name
    assert _lib.HIDDEN_SIGNATURES["ivit_hidden_f32"] == [P, P, F, I, I, I, I, I, P]
    assert _lib.HIDDEN_SIGNATURES["ivit_vit_hidden_scale"] == [P, I, P] == _lib.HIDDEN_SIGNATURES["ivit_swin_hidden_scale"]
    runner = [P, P, I, I, P, ctypes.c_size_t, P, P, I, P, I, P]
    for model in ("vit", "swin"):
        assert _lib.HIDDEN_SIGNATURES[f"ivit_{model}_hidden_states"] == runner
        assert _lib.HIDDEN_SIGNATURES[f"ivit_{model}_hidden_states_graph_create"] == runner + [P]
    versions = (_lib.IVIT_VERSION, _lib.IVIT_EVAL_VERSION, _lib.IVIT_FEATURES_VERSION, _lib.IVIT_ATTNMAP_VERSION, _lib.IVIT_CLASSMAP_VERSION)
    abis = (_lib.ABI, _lib.EVAL_ABI, _lib.FEATURES_ABI, _lib.ATTNMAP_ABI, _lib.CLASSMAP_ABI)
    older = set()
    for (name, (count, version, digest)), abi, v in zip(OLDER_HEADERS.items(), abis, versions):
        assert len(abi.functions) == count and v == version and _prototypes_digest(abi) == digest, name
        text = open(os.path.join(ROOT, "include", name)).read()
        assert _prototypes_digest(_abi.parse(text) if name == "ivit.h" else _abi.parse(text, base=_lib.ABI)) == digest, name
        assert "ivit_hidden" not in text and "hidden_states" not in text, name
        older |= set(abi.functions)
    assert not set(ENTRIES) & older
    with pytest.raises(_abi.AbiError):                    # it names handles of ivit.h: it parses only with ivit.h as its base
        _abi.parse(open(_abi.HIDDEN_HEADER).read())


def test_build_follows_the_hidden_header():
    so = iv.build()
    assert os.path.getmtime(so) >= os.path.getmtime(_abi.HIDDEN_HEADER)
    assert "ivit_hidden.h" in _lib.SOURCES and os.path.exists(os.path.join(ROOT, "i-vit_amd", "csrc", "ivit_hidden.h"))
    src = open(os.path.join(ROOT, "i-vit_amd", "_lib.py")).read()
    assert re.search(r"newest = max\(.*_abi\.ATTNMAP_HEADER, _abi\.CLASSMAP_HEADER, _abi\.HIDDEN_HEADER", src)


def test_hidden_states_on_both_engines():
    from ivit_amd.engine import ViTEngine
    from ivit_amd.native import NativeEngine
    from ivit_amd.swin_engine import SwinEngine
    for cls in (NativeEngine, ViTEngine, SwinEngine):
        assert all(hasattr(cls, n) for n in ("hidden_states", "capture_hidden_states", "hidden_scale_host")), cls
    assert ViTEngine.HIDDEN_CLASS_ROW and not SwinEngine.HIDDEN_CLASS_ROW
    import inspect
    assert list(inspect.signature(ViTEngine.hidden_states).parameters)[1:3] == ["images", "blocks"]
    assert list(inspect.signature(SwinEngine.hidden_states).parameters)[1:3] == ["images", "stages"]


# ---------------------------------------------------------------- the kernel in the code object
def test_hidden_kernels_in_code_object_without_scratch(tmp_path):
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
        lds = re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk)
        if nm and scratch and spill and lds:
            kernels[nm.group(1)] = (int(scratch.group(1)), int(spill.group(1)), int(lds.group(1)))
    assert len(kernels) > 100, "code object metadata looks wrong"
    want = sorted(k for k in kernels if re.fullmatch(r"_Z\d+hidden_f32_kernelILb[01]EE\w+", k))
    assert len(want) == 2 and "ILb0E" in want[0] and "ILb1E" in want[1], want       # TOKENS and GRID
    assert kernels[want[0]] == (0, 0, 0), kernels[want[0]]                          # the stream: no LDS
    assert kernels[want[1]] == (0, 0, 64 * 65 * 4), kernels[want[1]]               # the tile: 64 token rows at an odd pitch of 65 dwords
