"""The single-linkage hierarchy without a GPU: include/ivit_linkage.h declares three entries under version 1 and the binding follows
it; `Linkage.cut` on the edges of `predict.linkage_reference` against the components of `range_reference`'s pair list; `cut_k`."""
import ctypes
import os
import re
import numpy as np
from conftest import ROOT
import ivit_amd as iv
from ivit_amd import _abi, _lib
from ivit_amd.cluster import Linkage
from ivit_amd.predict import inv_norms_reference, linkage_reference, range_reference
from ivit_amd.search import duplicate_groups
from test_density_gpu import blobs

RUN = ["comp", "done", "edge_u", "edge_v", "edge_val", "state"]
ENTRIES = {"ivit_linkage_workspace_bytes": ["h", "rows", "dim", "splits", "bytes"], "ivit_linkage_init": ["h", "rows"] + RUN,
           "ivit_linkage_round": ["h", "x", "rows", "dim", "weight", "floor", "splits", "workspace", "bytes"] + RUN}


def test_linkage_header_declares_entries_and_the_binding_follows():
    hdr = open(os.path.join(ROOT, "include", "ivit_linkage.h")).read()
    assert re.search(r'#include "ivit\.h"', hdr)
    assert int(re.search(r"#define IVIT_LINKAGE_VERSION (\d+)", hdr).group(1)) == 1 == _lib.IVIT_LINKAGE_VERSION == _abi.LINKAGE_ABI.constants["IVIT_LINKAGE_VERSION"]
    assert {n: [p.name for p in f.params] for n, f in _abi.LINKAGE_ABI.functions.items()} == ENTRIES
    for name in ENTRIES:                                  # one "Alignment:" and one "Overlap:" line in front of every entry
        m = re.search(r"\bint %s\(" % name, hdr)
        front = hdr[hdr.rfind(";", 0, m.start()) + 1:m.start()]
        assert len(re.findall(r"\bAlignment:", front)) == 1 and len(re.findall(r"\bOverlap:", front)) == 1, name
    so = iv.build()
    assert os.path.getmtime(so) >= os.path.getmtime(_abi.LINKAGE_HEADER) and "ivit_linkage.h" in _lib.SOURCES
    lib = _lib.load()
    P, I, L, F, Z = _lib._P, _lib._I, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t
    assert _lib.LINKAGE_SIGNATURES == {"ivit_linkage_workspace_bytes": [P, L, I, I, P], "ivit_linkage_init": [P, L] + [P] * 6,
                                       "ivit_linkage_round": [P, P, L, I, P, F, I, P, Z] + [P] * 6}
    for name in ENTRIES:                                  # every bound name is exported
        assert getattr(lib, name).argtypes == _lib.LINKAGE_SIGNATURES[name] and _lib.LINKAGE_RESTYPES[name] is I, name


def test_cut_of_the_reference_tree_is_the_components_of_the_pair_list():
    x = blobs(300, 192)
    w = inv_norms_reference(x)
    tree = Linkage(*linkage_reference(x, w), 300)
    assert tree.u.shape[0] == 299 and bool((tree.u < tree.v).all()) and bool((tree.val[:-1] >= tree.val[1:]).all())
    low = float(np.finfo(np.float32).min)
    v = np.sort(range_reference(x, x, w, w, low, 0, 0, True)[2])
    for thr in (v[(len(v) * 9) // 10], v[-200]):          # values some pair attains exactly: >= on the boundary
        rp, idx, _ = range_reference(x, x, w, w, thr, 0, 0, True)
        pairs = np.stack([np.repeat(np.arange(300), np.diff(rp)), idx.astype(np.int64)], 1)
        want = duplicate_groups(pairs, 300)
        assert np.array_equal(tree.cut(thr), want) and 1 < len(np.unique(want)) < 300, float(thr)
        floored = Linkage(*linkage_reference(x, w, thr), 300)            # the forest above a floor: the same edges, the same groups
        n = floored.u.shape[0]
        assert n == 300 - len(np.unique(want)) and all(np.array_equal(a[:n], b) for a, b in zip((tree.u, tree.v, tree.val), (floored.u, floored.v, floored.val)))


def test_cut_k_and_matrix():
    x = blobs(97, 64)
    tree = Linkage(*linkage_reference(x, None), 97)
    assert np.array_equal(tree.cut_k(1), np.zeros(97, np.int64)) and np.array_equal(tree.cut_k(97), np.arange(97))
    assert len(np.unique(tree.cut_k(5))) == 5
    Z = tree.matrix()
    assert Z.shape == (96, 4) and Z.dtype == np.float64 and Z[-1, 3] == 97 and (np.diff(Z[:, 2]) >= 0).all() and (Z[:, 0] < Z[:, 1]).all()
    assert sorted(Z[:, :2].astype(np.int64).ravel().tolist()) == list(range(2 * 96))       # every row and every cluster but the last joins once


# ---------------------------------------------------------------- the kernels in the code object
def test_linkage_kernels_in_code_object_without_scratch(tmp_path):
    from test_search_cpu import check_scan_kernels_in_code_object
    # the plain round and the mutual-reachability round; the core values are prefetched wherever the tile is
    check_scan_kernels_in_code_object(tmp_path, "linkage_scan_kernel", ["Li0E", "Li1E"], second_pf=True)
