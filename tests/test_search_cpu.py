"""Gallery search without a GPU: include/ivit_search.h declares four entries under version 1 beside six unchanged headers, the binding
follows it and the build its mtime; `search_reference` is `topk_reference` on the dot products wherever both apply;
`inv_norms_reference` is 1 / sqrt in float64 rounded once; `knn_reference` on a hand-written case with a vote tie; and the new
kernels are in the gfx950 code object without scratch."""
import ctypes
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import ivit_amd as iv
from ivit_amd import _abi, _lib
from ivit_amd.predict import inv_norms_reference, search_reference, topk_reference

ENTRIES = {"ivit_gallery_inv_norms": 5, "ivit_search_workspace_bytes": 7, "ivit_search_topk": 14, "ivit_search_merge": 8}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- the seventh header and its binding
def test_search_header_declares_entries_and_version():
    hdr = open(os.path.join(ROOT, "include", "ivit_search.h")).read()
    assert re.search(r'#include "ivit\.h"', hdr)
    assert int(re.search(r"#define IVIT_SEARCH_VERSION (\d+)", hdr).group(1)) == 1 == _lib.IVIT_SEARCH_VERSION
    assert _abi.SEARCH_ABI.constants == {"IVIT_SEARCH_VERSION": 1}
    assert list(_abi.SEARCH_ABI.functions) == list(ENTRIES)
    for name in ENTRIES:                                  # one "Alignment:" and one "Overlap:" line in front of every entry
        m = re.search(r"\bint %s\(" % name, hdr)
        front = hdr[hdr.rfind(";", 0, m.start()) + 1:m.start()]
        assert len(re.findall(r"\bAlignment:", front)) == 1 and len(re.findall(r"\bOverlap:", front)) == 1, name
    assert re.search(r"int\s+ivit_gallery_inv_norms\s*\(\s*ivit_handle\s+h\s*,\s*const\s+int8_t\s*\*\s*gallery\s*,\s*int64_t\s+rows\s*,\s*int\s+dim\s*,"
                     r"\s*float\s*\*\s*inv_norm\s*\)", hdr)
    assert re.search(r"int\s+ivit_search_workspace_bytes\s*\(\s*ivit_handle\s+h\s*,\s*int\s+nq\s*,\s*int64_t\s+rows\s*,\s*int\s+dim\s*,\s*int\s+k\s*,"
                     r"\s*int\s+splits\s*,\s*size_t\s*\*\s*bytes\s*\)", hdr)
    assert re.search(r"int\s+ivit_search_topk\s*\(\s*ivit_handle\s+h\s*,\s*const\s+int8_t\s*\*\s*query\s*,\s*int\s+nq\s*,\s*const\s+int8_t\s*\*\s*gallery\s*,"
                     r"\s*int64_t\s+rows\s*,\s*int\s+dim\s*,\s*const\s+float\s*\*\s*weight\s*,\s*int\s+k\s*,\s*int32_t\s+index_base\s*,\s*int\s+splits\s*,"
                     r"\s*void\s*\*\s*workspace\s*,\s*size_t\s+bytes\s*,\s*int32_t\s*\*\s*idx\s*,\s*float\s*\*\s*val\s*\)", hdr)
    assert re.search(r"int\s+ivit_search_merge\s*\(\s*ivit_handle\s+h\s*,\s*const\s+int32_t\s*\*\s*idx_in\s*,\s*const\s+float\s*\*\s*val_in\s*,\s*int\s+nq\s*,"
                     r"\s*int\s+ncand\s*,\s*int\s+k\s*,\s*int32_t\s*\*\s*idx\s*,\s*float\s*\*\s*val\s*\)", hdr)


# the six older headers: prototype count, version and sha256 of their prototypes (names, parameter types and names, in order).  The
# first five digests are those test_hidden_cpu.py pins; ivit_hidden.h's was computed with the same function on the parent commit
OLDER_HEADERS = {"ivit.h": (99, 111, "6817c4e822691347e82f51942395393d315550b28b44df8fd32f8d739abd6b52"),
                 "ivit_eval.h": (5, 1, "b47eee22a4d967fa3efca30b6994987eecccbe61cf040a3608941660bf3bee07"),
                 "ivit_features.h": (5, 1, "cb523d76e256d935c2b277e969372ad9fbcde8cbdb97559fa7d84a6516f2159f"),
                 "ivit_attnmap.h": (4, 1, "2f429e1f49a79e9a910707d666d5d274831c1f49f0e8177fd51abf43952572f6"),
                 "ivit_classmap.h": (3, 1, "8da355354133cbf09e4e986c0bb6e4081b79ba6c60ac3fdb746cceec64bc3620"),
                 "ivit_hidden.h": (7, 1, "e32b2dd1cfd7fa95a32729c1e3b888b5f32d46680928bf55b727671ba8d2f93f")}


def _prototypes_digest(abi):
    text = "\n".join(name + "(" + ", ".join(re.sub(r"\s+", " ", d.type) + " " + d.name for d in f.params) + ")"
                     for name, f in abi.functions.items())
    return hashlib.sha256(text.encode()).hexdigest()


def test_search_entries_bound_and_exported_beside_unchanged_headers():
    iv.build()
    lib = _lib.load()
    P, I, L, Z = _lib._P, _lib._I, ctypes.c_int64, ctypes.c_size_t
    assert list(_lib.SEARCH_SIGNATURES) == list(ENTRIES) == list(_lib.SEARCH_RESTYPES)
    for name, nparams in ENTRIES.items():             # every bound name is exported, with the header's parameter count
        bound = getattr(lib, name)
        assert len(_lib.SEARCH_SIGNATURES[name]) == nparams and bound.argtypes == _lib.SEARCH_SIGNATURES[name] and bound.restype is I, name
    assert _lib.SEARCH_SIGNATURES["ivit_gallery_inv_norms"] == [P, P, L, I, P]
    assert _lib.SEARCH_SIGNATURES["ivit_search_workspace_bytes"] == [P, I, L, I, I, I, P]
    assert _lib.SEARCH_SIGNATURES["ivit_search_topk"] == [P, P, I, P, L, I, P, I, ctypes.c_int32, I, P, Z, P, P]
    assert _lib.SEARCH_SIGNATURES["ivit_search_merge"] == [P, P, P, I, I, I, P, P]
    versions = (_lib.IVIT_VERSION, _lib.IVIT_EVAL_VERSION, _lib.IVIT_FEATURES_VERSION, _lib.IVIT_ATTNMAP_VERSION, _lib.IVIT_CLASSMAP_VERSION,
                _lib.IVIT_HIDDEN_VERSION)
    abis = (_lib.ABI, _lib.EVAL_ABI, _lib.FEATURES_ABI, _lib.ATTNMAP_ABI, _lib.CLASSMAP_ABI, _lib.HIDDEN_ABI)
    older = set()
    for (name, (count, version, digest)), abi, v in zip(OLDER_HEADERS.items(), abis, versions):
        assert len(abi.functions) == count and v == version and _prototypes_digest(abi) == digest, name
        text = open(os.path.join(ROOT, "include", name)).read()
        assert _prototypes_digest(_abi.parse(text) if name == "ivit.h" else _abi.parse(text, base=_lib.ABI)) == digest, name
        assert "ivit_search" not in text and "ivit_gallery" not in text, name
        older |= set(abi.functions)
    assert not set(ENTRIES) & older
    with pytest.raises(_abi.AbiError):                    # it names a handle of ivit.h: it parses only with ivit.h as its base
        _abi.parse(open(_abi.SEARCH_HEADER).read())


def test_build_follows_the_search_header():
    so = iv.build()
    assert os.path.getmtime(so) >= os.path.getmtime(_abi.SEARCH_HEADER)
    assert "ivit_search.h" in _lib.SOURCES and os.path.exists(os.path.join(ROOT, "i-vit_amd", "csrc", "ivit_search.h"))
    src = open(os.path.join(ROOT, "i-vit_amd", "_lib.py")).read()
    assert re.search(r"newest = max\(.*_abi\.HIDDEN_HEADER, _abi\.SEARCH_HEADER", src)


def test_retrieve_on_both_engines():
    import inspect
    from ivit_amd import predict, search
    from ivit_amd.engine import ViTEngine
    from ivit_amd.native import NativeEngine
    from ivit_amd.swin_engine import SwinEngine
    for cls in (NativeEngine, ViTEngine, SwinEngine):
        assert list(inspect.signature(cls.retrieve).parameters)[1:5] == ["images", "gallery", "k", "nslices"], cls
    assert list(inspect.signature(search.Gallery.__init__).parameters)[1:5] == ["feat8", "labels", "cosine", "chunk_rows"]
    assert list(inspect.signature(search.knn_classify).parameters) == ["idx", "val", "labels", "num_classes", "T", "query_inv_norm"]
    assert list(inspect.signature(predict.knn_evaluate).parameters) == ["engine", "gallery", "batches", "k", "T", "topk", "transform"]
    assert list(inspect.signature(predict.embed8).parameters) == ["engine", "batches", "transform"]
    assert predict.MAX_K == 16 and predict.SEARCH_MAX_K == 64 == search.MAX_K


# ---------------------------------------------------------------- the numpy statements
@pytest.mark.parametrize("lo,hi", [(-3, 4), (-128, 128)])
def test_search_reference_is_topk_reference_on_the_dot_products(lo, hi):
    rng = np.random.default_rng(11)
    q = rng.integers(lo, hi, size=(5, 64)).astype(np.int8)
    g = rng.integers(lo, hi, size=(300, 64)).astype(np.int8)
    acc = q.astype(np.int32) @ g.astype(np.int32).T
    w = inv_norms_reference(g)
    for k in (1, 7, 16):
        for weight, scale in ((None, np.ones(300, np.float32)), (w, w)):
            idx, val = search_reference(q, g, weight, k)
            ridx, rval = topk_reference(acc, scale, k)
            assert idx.dtype == np.int32 and val.dtype == np.float32 and idx.shape == val.shape == (5, k)
            assert np.array_equal(idx, ridx) and np.array_equal(bits(val), bits(rval))
    idx0, val0 = search_reference(q, g, w, 16)
    idxb, valb = search_reference(q, g, w, 16, index_base=2 ** 31 - 1 - 300)
    assert np.array_equal(idxb.astype(np.int64) - idx0, np.full((5, 16), 2 ** 31 - 1 - 300)) and np.array_equal(bits(val0), bits(valb))
    assert search_reference(q, g, None, 64)[0].shape == (5, 64)         # beyond topk_reference's 16
    assert np.array_equal(search_reference(q, g, None, 64)[0][:, :16], search_reference(q, g, None, 16)[0])
    for bad in (0, 65, 301):
        with pytest.raises(ValueError):
            search_reference(q, g[:300], None, bad)
    with pytest.raises(ValueError):
        search_reference(q, g[:10], None, 11)
    with pytest.raises(ValueError):
        search_reference(q, g, None, 1, index_base=2 ** 31 - 300)
    with pytest.raises(ValueError):
        search_reference(q, g, None, 1, index_base=-1)


def test_search_reference_ties_and_signed_zeros():
    """equal values come by ascending index; -0.0 ties +0.0 and keeps its sign in val"""
    g = np.zeros((6, 64), np.int8)
    g[:, 0] = [1, -1, 1, -1, 0, 2]
    q = np.zeros((1, 64), np.int8)
    q[0, 0] = 3
    w = np.array([0.0, 0.0, -0.0, -0.0, 1.0, 0.5], np.float32)         # values +0, -0, -0, +0, 0 * 1 = +0, 3
    idx, val = search_reference(q, g, w, 6)
    assert idx.tolist() == [[5, 0, 1, 2, 3, 4]]
    assert bits(val).tolist() == [[0x40400000, 0, 0x80000000, 0x80000000, 0, 0]]
    one = np.repeat(g[:1], 9, axis=0)
    assert search_reference(q, one, None, 4, index_base=10)[0].tolist() == [[10, 11, 12, 13]]


def test_inv_norms_reference():
    rng = np.random.default_rng(5)
    g = rng.integers(-128, 128, size=(200, 192)).astype(np.int8)
    g[0] = 0
    g[1] = -128
    g[2] = 0
    g[2, 7] = 1
    inv = inv_norms_reference(g)
    assert inv.dtype == np.float32 and inv.shape == (200,)
    ss = (g.astype(np.int64) ** 2).sum(1)
    want = np.zeros(200, np.float32)
    want[ss > 0] = (np.float64(1.0) / np.sqrt(ss[ss > 0].astype(np.float64))).astype(np.float32)     # float64 throughout, rounded once
    assert np.array_equal(bits(inv), bits(want))
    assert bits(inv)[0] == 0 and inv[2] == 1.0 and inv[1] == np.float32(1.0 / np.sqrt(192 * 16384.0))
    # a row against itself: fl32(fl32(ss) * inv_norm) is |g| within one ulp (a statement about the reference, not a tolerance on a kernel)
    for dim in (64, 192, 1024):
        g = rng.integers(-128, 128, size=(500, dim)).astype(np.int8)
        ss = (g.astype(np.int64) ** 2).sum(1)
        assert ss.max() <= 2 ** 24
        v = ss.astype(np.float32) * inv_norms_reference(g)
        # inv_norm is 1 / |g| within half an ulp and the product rounds once more: under 1.5 ulp from |g|, so at most ONE float32
        # step from |g| rounded to float32
        norm32 = np.sqrt(ss.astype(np.float64)).astype(np.float32)
        assert np.all(np.abs(v.astype(np.float64) - norm32.astype(np.float64)) <= np.spacing(norm32).astype(np.float64))


def test_knn_reference_hand_written_case_with_a_vote_tie():
    from ivit_amd.search import knn_reference
    labels = np.array([2, 0, 2, 1, 0], np.int64)
    # query 0: neighbours 0 (class 2), 1 (class 0), 3 (class 1) with cosines 0.7, 0.7, 0.35: classes 0 and 2 tie, class 0 comes first
    # query 1: neighbours 2 (class 2), 0 (class 2), 4 (class 0): class 2 has two votes
    idx = np.array([[0, 1, 3], [2, 0, 4]], np.int32)
    val = np.array([[0.7, 0.7, 0.35], [0.5, 0.25, 0.6]], np.float32)
    order, vote = knn_reference(idx, val, labels, 4, T=0.07)
    e = lambda c: np.exp(np.float64(np.float32(c)) / 0.07)      # noqa: E731
    assert vote.dtype == np.float64 and vote.shape == (2, 4) and order.dtype == np.int64
    assert vote[0].tolist() == [e(0.7), e(0.35), e(0.7), 0.0]
    assert order[0].tolist() == [0, 2, 1, 3]                    # the tie of classes 0 and 2 by class index; the empty class last
    assert vote[1].tolist() == [e(0.6), 0.0, e(0.5) + e(0.25), 0.0]
    assert e(0.6) > e(0.5) + e(0.25) and order[1].tolist() == [0, 2, 1, 3]      # one near neighbour outvotes two far ones at T = 0.07
    # with the queries' inverse norms the cosines shrink and so do the votes; a different T changes the weights, not who voted
    order2, vote2 = knn_reference(idx, val, labels, 4, T=0.07, query_inv_norm=np.array([0.5, 1.0]))
    h = lambda c: np.exp(np.float64(np.float32(c)) * 0.5 / 0.07)      # noqa: E731
    assert vote2[0].tolist() == [h(0.7), h(0.35), h(0.7), 0.0]
    assert np.array_equal(vote2[1], vote[1]) and np.array_equal(order2, order)
    assert (knn_reference(idx, val, labels, 4, T=1.0)[1] > 0).tolist() == (vote > 0).tolist()


# ---------------------------------------------------------------- the kernels in the code object
def test_search_kernels_in_code_object_without_scratch(tmp_path):
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
    scan = sorted(k for k in kernels if re.fullmatch(r"_Z\d+search_scan_kernelILi\d+ELb[01]EE\w+", k))
    widths = sorted(int(re.search(r"ILi(\d+)E", k).group(1)) for k in scan)
    assert widths == list(range(1, 17)), widths                     # dim = 64 .. 1024 in steps of 64, one instantiation each
    for k in scan:                                                  # the next tile is prefetched up to dim 512
        assert ("ELb1E" in k) == (int(re.search(r"ILi(\d+)E", k).group(1)) <= 8), k
    select = sorted(k for k in kernels if re.fullmatch(r"_Z\d+search_select_kernelILb[01]ELi(0|16|64)EE\w+", k))
    norms = [k for k in kernels if re.fullmatch(r"_Z\d+gallery_inv_norms_kernel\w+", k)]
    assert len(select) == 6 and len(norms) == 1, (select, norms)     # keys or (val, idx) pairs x 16 / 64 keys per lane in registers / rescanned
    for k in scan + select + norms:                                 # no scratch, no spills; the candidate slots are dynamic LDS
        assert kernels[k] == (0, 0, 0), (k, kernels[k])
