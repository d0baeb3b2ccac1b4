"""Density clustering without a GPU: include/ivit_density.h declares five entries under version 1 and the binding follows it;
`predict.dbscan_reference` on a hand-written graph with a known answer, and at min_pts = 1 against `search.duplicate_groups` on the
pairs of `range_reference`."""
import ctypes
import os
import re
import numpy as np
import pytest
from conftest import ROOT
import ivit_amd as iv
from ivit_amd import _abi, _lib
from ivit_amd.predict import dbscan_reference, inv_norms_reference, range_reference
from ivit_amd.search import duplicate_groups

SCAN = ["h", "x", "rows", "dim", "weight", "threshold", "splits", "workspace", "bytes"]
ENTRIES = {"ivit_density_workspace_bytes": ["h", "rows", "dim", "splits", "bytes"],
           "ivit_density_degree": SCAN + ["degree"], "ivit_density_init": ["h", "degree", "rows", "min_pts", "label", "dirty"],
           "ivit_density_sweep": SCAN + ["label_in", "dirty_in", "label_out", "dirty_out", "changed"],
           "ivit_density_border": SCAN + ["label", "out"]}


def test_density_header_declares_entries_and_the_binding_follows():
    hdr = open(os.path.join(ROOT, "include", "ivit_density.h")).read()
    assert re.search(r'#include "ivit\.h"', hdr)
    assert int(re.search(r"#define IVIT_DENSITY_VERSION (\d+)", hdr).group(1)) == 1 == _lib.IVIT_DENSITY_VERSION == _abi.DENSITY_ABI.constants["IVIT_DENSITY_VERSION"]
    assert {n: [p.name for p in f.params] for n, f in _abi.DENSITY_ABI.functions.items()} == ENTRIES
    for name in ENTRIES:                                  # one "Alignment:" and one "Overlap:" line in front of every entry
        m = re.search(r"\bint %s\(" % name, hdr)
        front = hdr[hdr.rfind(";", 0, m.start()) + 1:m.start()]
        assert len(re.findall(r"\bAlignment:", front)) == 1 and len(re.findall(r"\bOverlap:", front)) == 1, name
    so = iv.build()
    assert os.path.getmtime(so) >= os.path.getmtime(_abi.DENSITY_HEADER) and "ivit_density.h" in _lib.SOURCES
    lib = _lib.load()
    P, I, L, F, Z = _lib._P, _lib._I, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t
    scan = [P, P, L, I, P, F, I, P, Z]
    assert _lib.DENSITY_SIGNATURES == {"ivit_density_workspace_bytes": [P, L, I, I, P], "ivit_density_degree": scan + [P],
                                       "ivit_density_init": [P, P, L, ctypes.c_int32, P, P], "ivit_density_sweep": scan + [P] * 5,
                                       "ivit_density_border": scan + [P, P]}
    for name in ENTRIES:                                  # every bound name is exported
        assert getattr(lib, name).argtypes == _lib.DENSITY_SIGNATURES[name] and _lib.DENSITY_RESTYPES[name] is I, name


def test_dbscan_reference_on_a_hand_written_graph():
    """every edge owns a column in which both its rows hold 3, so a pair's dot product is 9 on an edge and 0 elsewhere, and a row's own
    is 9 per column it holds: at a threshold of 9 every row but the empty one counts itself.  Rows 0 1 2 and 5 6 7 are triangles;
    row 3 is adjacent to 1 and to 5; row 4 is empty; row 8 holds a column of its own and has no neighbour but itself"""
    edges = [(0, 1), (0, 2), (1, 2), (5, 6), (5, 7), (6, 7), (3, 1), (3, 5), (8, 8)]
    x = np.zeros((9, 64), np.int8)
    for c, (i, j) in enumerate(edges):
        x[i, c] = x[j, c] = 3
    label, core, degree = dbscan_reference(x, None, 9, 4)
    assert degree.tolist() == [3, 4, 3, 3, 0, 4, 3, 3, 1] and degree.dtype == np.int32 and label.dtype == np.int32
    assert core.tolist() == [False, True, False, False, False, True, False, False, False]      # core only because they count themselves
    assert label.tolist() == [1, 1, 1, 1, -1, 5, 5, 5, -1]            # two clusters; border row 3 sees 1 and 5 and takes 1; 4 and 8 noise
    assert dbscan_reference(x, None, 9, 3)[0].tolist() == [0, 0, 0, 0, -1, 0, 0, 0, -1]        # row 3 is core now and joins the two
    assert dbscan_reference(x, None, 9, 1)[0].tolist() == [0, 0, 0, 0, -1, 0, 0, 0, 8]         # the empty row does not even pass itself
    w = np.array([1, 4, 1, 1, 1, 0.25, 1, 1, 1], np.float32)          # exact powers of two: row 5 reaches neither 3, 6, 7 nor itself
    label, core, degree = dbscan_reference(x, w, 9, 4)
    assert degree.tolist() == [3, 4, 3, 2, 0, 0, 2, 2, 1] and label.tolist() == [1, 1, 1, 1, -1, -1, -1, -1, -1]
    for thr, min_pts in ((np.inf, 1), (np.nan, 1), (1.0, 0)):
        with pytest.raises(ValueError):
            dbscan_reference(x, None, thr, min_pts)


@pytest.mark.parametrize("cosine", [False, True])
def test_dbscan_reference_at_min_pts_1_is_duplicate_groups(cosine):
    rng = np.random.default_rng(3)
    x = (rng.integers(-3, 4, size=(6, 64))[rng.integers(0, 6, size=70)] + rng.integers(-1, 2, size=(70, 64))).astype(np.int8)
    w = inv_norms_reference(x) if cosine else None
    v = range_reference(x, x, w, w, float(np.finfo(np.float32).min), 0, 0, True)[2]
    for thr in (np.float32(np.percentile(v, 60)), np.float32(np.percentile(v, 90)), v[len(v) // 2]):
        rp, idx, _ = range_reference(x, x, w, w, thr, 0, 0, True)
        pairs = np.stack([np.repeat(np.arange(70), np.diff(rp)), idx.astype(np.int64)], 1)
        label, core, degree = dbscan_reference(x, w, thr, 1)
        # a row without a neighbour that misses the threshold itself (dot product only) has degree 0: noise here, its own group there
        assert np.array_equal(core, degree >= 1) and (core.all() or not cosine), float(thr)
        assert np.array_equal(np.where(label < 0, np.arange(70), label), duplicate_groups(pairs, 70)), float(thr)
    assert 1 < len(np.unique(dbscan_reference(x, w, np.float32(np.percentile(v, 90)), 1)[0])) < 70


# ---------------------------------------------------------------- the kernels in the code object
def test_density_kernels_in_code_object_without_scratch(tmp_path):
    from test_search_cpu import check_scan_kernels_in_code_object
    check_scan_kernels_in_code_object(tmp_path, "density_scan_kernel", ["Li0E", "Li1E", "Li2E"])        # degree, sweep, border
