"""Range search without a GPU: include/ivit_range.h declares three entries under version 1 beside eleven unchanged headers, the binding
follows it and the build its mtime; `predict.range_reference` against a three-loop brute force, against `search_reference` at
k = rows (the cross-statement the header names) and, with the triangle, in chunk pairs against the one-piece self-join;
`search.duplicate_groups` against a breadth-first search."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import ivit_amd as iv
from ivit_amd import _abi, _lib
from ivit_amd.predict import inv_norms_reference, range_reference, search_reference
from test_cluster_cpu import OLDER_HEADERS as TEN_OLDER
from test_search_cpu import _prototypes_digest

ENTRIES = {"ivit_range_workspace_bytes": 6, "ivit_range_count": 16, "ivit_range_fill": 18}

# the eleven older headers: prototype count, version and sha256 of their prototypes.  The first ten are those test_cluster_cpu.py
# pins; ivit_cluster.h's was computed with the same function on the parent commit
OLDER_HEADERS = dict(TEN_OLDER, **{"ivit_cluster.h": (4, 1, "2759cd3a2144a22df5659731406730f9d2dc450620b1bf7779efb2a39f28870b")})


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- the twelfth header and its binding
def test_range_header_declares_entries_and_version():
    hdr = open(os.path.join(ROOT, "include", "ivit_range.h")).read()
    assert re.search(r'#include "ivit\.h"', hdr)
    assert int(re.search(r"#define IVIT_RANGE_VERSION (\d+)", hdr).group(1)) == 1 == _lib.IVIT_RANGE_VERSION
    assert _abi.RANGE_ABI.constants == {"IVIT_RANGE_VERSION": 1}
    assert list(_abi.RANGE_ABI.functions) == list(ENTRIES)
    for name in ENTRIES:                                  # one "Alignment:" and one "Overlap:" line in front of every entry
        m = re.search(r"\bint %s\(" % name, hdr)
        front = hdr[hdr.rfind(";", 0, m.start()) + 1:m.start()]
        assert len(re.findall(r"\bAlignment:", front)) == 1 and len(re.findall(r"\bOverlap:", front)) == 1, name
    fns = _abi.RANGE_ABI.functions
    common = ["h", "query", "nq", "gallery", "rows", "dim", "weight", "qweight", "threshold", "index_base", "query_base", "triangle", "splits",
              "workspace", "bytes"]
    assert [p.name for p in fns["ivit_range_workspace_bytes"].params] == ["h", "nq", "rows", "dim", "splits", "bytes"]
    assert [p.name for p in fns["ivit_range_count"].params] == common + ["row_ptr"]
    assert [p.name for p in fns["ivit_range_fill"].params] == common + ["capacity", "idx", "val"]


def test_range_entries_bound_and_exported_beside_unchanged_headers():
    iv.build()
    lib = _lib.load()
    P, I, L, F, Z = _lib._P, _lib._I, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t
    assert list(_lib.RANGE_SIGNATURES) == list(ENTRIES) == list(_lib.RANGE_RESTYPES)
    for name, nparams in ENTRIES.items():             # every bound name is exported, with the header's parameter count
        bound = getattr(lib, name)
        assert len(_lib.RANGE_SIGNATURES[name]) == nparams and bound.argtypes == _lib.RANGE_SIGNATURES[name] and bound.restype is I, name
    common = [P, P, I, P, L, I, P, P, F, ctypes.c_int32, ctypes.c_int32, I, I, P, Z]
    assert _lib.RANGE_SIGNATURES["ivit_range_workspace_bytes"] == [P, I, L, I, I, P]
    assert _lib.RANGE_SIGNATURES["ivit_range_count"] == common + [P]
    assert _lib.RANGE_SIGNATURES["ivit_range_fill"] == common + [L, P, P]
    versions = (_lib.IVIT_VERSION, _lib.IVIT_EVAL_VERSION, _lib.IVIT_FEATURES_VERSION, _lib.IVIT_ATTNMAP_VERSION, _lib.IVIT_CLASSMAP_VERSION,
                _lib.IVIT_HIDDEN_VERSION, _lib.IVIT_SEARCH_VERSION, _lib.IVIT_MODELFILE_VERSION, _lib.IVIT_PROBE_VERSION, _lib.IVIT_VIEWS_VERSION,
                _lib.IVIT_CLUSTER_VERSION)
    abis = (_lib.ABI, _lib.EVAL_ABI, _lib.FEATURES_ABI, _lib.ATTNMAP_ABI, _lib.CLASSMAP_ABI, _lib.HIDDEN_ABI, _lib.SEARCH_ABI, _lib.MODELFILE_ABI,
            _lib.PROBE_ABI, _lib.VIEWS_ABI, _lib.CLUSTER_ABI)
    assert len(OLDER_HEADERS) == 11 == len(abis)
    older = set()
    for (name, (count, version, digest)), abi, v in zip(OLDER_HEADERS.items(), abis, versions):
        assert len(abi.functions) == count and v == version and _prototypes_digest(abi) == digest, name
        text = open(os.path.join(ROOT, "include", name)).read()
        assert _prototypes_digest(_abi.parse(text) if name == "ivit.h" else _abi.parse(text, base=_lib.ABI)) == digest, name
        assert "ivit_range" not in text, name
        older |= set(abi.functions)
    assert not set(ENTRIES) & older
    with pytest.raises(_abi.AbiError):                    # it names a handle of ivit.h: it parses only with ivit.h as its base
        _abi.parse(open(_abi.RANGE_HEADER).read())


def test_build_follows_the_range_header():
    so = iv.build()
    assert os.path.getmtime(so) >= os.path.getmtime(_abi.RANGE_HEADER)
    assert "ivit_range.h" in _lib.SOURCES and os.path.exists(os.path.join(ROOT, "i-vit_amd", "csrc", "ivit_range.h"))
    src = open(os.path.join(ROOT, "i-vit_amd", "_lib.py")).read()
    assert re.search(r"newest = max\(.*_abi\.CLUSTER_HEADER, _abi\.RANGE_HEADER", src)
    hip = open(os.path.join(ROOT, "i-vit_amd", "csrc", "ivit_hip.hip")).read()
    assert '#include "ivit_range.h"' in hip


def test_range_python_layer_is_there_on_both_engines():
    from ivit_amd import predict, search
    from ivit_amd.engine import ViTEngine
    from ivit_amd.native import NativeEngine
    from ivit_amd.swin_engine import SwinEngine
    for cls in (NativeEngine, ViTEngine, SwinEngine):
        assert list(inspect.signature(cls.retrieve_within).parameters)[1:4] == ["images", "gallery", "threshold"], cls
    assert list(inspect.signature(search.Gallery.within).parameters) == ["self", "query8", "threshold", "query_weight", "triangle", "query_base"]
    assert list(inspect.signature(predict.range_reference).parameters) == ["query8", "gallery8", "weight", "qweight", "threshold", "index_base",
                                                                           "query_base", "triangle"]
    assert list(inspect.signature(predict.find_duplicates).parameters) == ["engine", "batches", "threshold", "transform"]
    assert list(inspect.signature(search.duplicates).parameters)[:3] == ["feat8", "threshold", "cosine"]
    assert list(inspect.signature(search.cross_matches).parameters)[:4] == ["feat8_a", "feat8_b", "threshold", "cosine"]
    assert "synchronis" in search.Gallery.within.__doc__.lower()          # the one host round trip is said where a caller reads


# ---------------------------------------------------------------- the numpy statement
def _brute(q, g, w, qw, thr, ib, qb, tri):
    """three loops, one scalar float32 operation at a time"""
    row_ptr, idx, val = [0], [], []
    for b in range(q.shape[0]):
        for r in range(g.shape[0]):
            dot = 0
            for c in range(q.shape[1]):
                dot += int(q[b, c]) * int(g[r, c])
            v = np.float32(dot)
            if w is not None:
                v = np.float32(v * np.float32(w[r]))
            if qw is not None:
                v = np.float32(v * np.float32(qw[b]))
            if v >= np.float32(thr) and (not tri or ib + r > qb + b):
                idx.append(ib + r)
                val.append(v)
        row_ptr.append(len(idx))
    return np.array(row_ptr, np.int64), np.array(idx, np.int32), np.array(val, np.float32)


def _small(seed, nq, rows, dim=8, lim=3):
    rng = np.random.default_rng(seed)
    return (rng.integers(-lim, lim + 1, size=(nq, dim)).astype(np.int8), rng.integers(-lim, lim + 1, size=(rows, dim)).astype(np.int8))


@pytest.mark.parametrize("seed", range(4))
def test_range_reference_is_the_three_loop_brute_force(seed):
    q, g = _small(seed, 5, 11)
    g[3] = 0                                              # a row of zeros: weight +0.0, v = +-0
    q[1] = 0
    w, qw = inv_norms_reference(g), inv_norms_reference(q)
    w[5] = -w[5]                                          # a negative weight: -0.0 where the dot product is 0
    hits = 0
    for weights in ((None, None), (w, None), (w, qw)):
        v = (q.astype(np.int32) @ g.astype(np.int32).T).astype(np.float32)
        v = v if weights[0] is None else v * weights[0][None, :]
        v = v if weights[1] is None else v * weights[1][:, None]
        for thr in (float(v.min()) - 1, float(v.max()) + 1, float(np.median(v)), 0.0, -0.0, float(v[2, 7])):
            for ib, qb, tri in ((0, 0, False), (7, 0, False), (0, 0, True), (3, 5, True), (5, 3, True), (2 ** 31 - 1 - 11, 2 ** 31 - 1 - 5, True)):
                got = range_reference(q, g, weights[0], weights[1], thr, ib, qb, tri)
                want = _brute(q, g, weights[0], weights[1], thr, ib, qb, tri)
                assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float32
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(bits(got[2]), bits(want[2]))
                hits += len(got[1])
    assert hits > 0
    rp, idx, val = range_reference(q, g, w, None, 0.0)
    assert (bits(val) == 0x80000000).any() and (bits(val) == 0).any()             # both zeros are hits at +0.0, the sign kept
    assert np.array_equal(bits(range_reference(q, g, w, None, -0.0)[2]), bits(val))
    for bad in (np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError):
            range_reference(q, g, None, None, bad)
    with pytest.raises(ValueError):
        range_reference(q, g, None, None, 0.0, index_base=2 ** 31 - 11)
    with pytest.raises(ValueError):
        range_reference(q, g, None, None, 0.0, query_base=-1)


@pytest.mark.parametrize("weighted", [False, True])
def test_range_reference_is_the_search_reference_cut_at_the_threshold(weighted):
    """qweight None, k = rows: a row of the result holds exactly the entries of the ranked list with a value >= threshold, by index"""
    q, g = _small(11, 7, 40, dim=16)
    w = inv_norms_reference(g) if weighted else None
    si, sv = search_reference(q, g, w, 40, index_base=9)
    for thr in (float(np.median(sv)), float(sv[0, 3]), 0.0, float(sv.max()) + 1):
        rp, idx, val = range_reference(q, g, w, None, thr, index_base=9)
        for b in range(7):
            keep = sv[b] >= np.float32(thr)
            order = np.argsort(si[b][keep], kind="stable")
            assert np.array_equal(idx[rp[b]:rp[b + 1]], si[b][keep][order])
            assert np.array_equal(bits(val[rp[b]:rp[b + 1]]), bits(sv[b][keep][order]))
    assert rp[-1] == 0                                    # above the maximum: nothing


def test_triangle_in_chunk_pairs_is_the_one_piece_self_join():
    x, _ = _small(5, 23, 1, dim=16, lim=2)
    x[9], x[17] = x[2], x[2]                              # planted duplicates
    w = inv_norms_reference(x)
    thr = 0.5
    rp, idx, val = range_reference(x, x, w, w, thr, 0, 0, True)
    whole = {(b, int(j)): int(v) for b in range(23) for j, v in zip(idx[rp[b]:rp[b + 1]], bits(val[rp[b]:rp[b + 1]]))}
    assert whole and all(i < j for i, j in whole) and (2, 9) in whole and (9, 17) in whole and (2, 17) in whole
    for cuts in ([0, 23], [0, 8, 23], [0, 5, 6, 16, 23]):
        got = {}
        for a0, a1 in zip(cuts[:-1], cuts[1:]):
            for b0, b1 in zip(cuts[:-1], cuts[1:]):
                crp, cidx, cval = range_reference(x[a0:a1], x[b0:b1], w[b0:b1], w[a0:a1], thr, b0, a0, True)
                for b in range(a1 - a0):
                    for j, v in zip(cidx[crp[b]:crp[b + 1]], bits(cval[crp[b]:crp[b + 1]])):
                        assert (a0 + b, int(j)) not in got
                        got[(a0 + b, int(j))] = int(v)
                if b1 - 1 <= a0:
                    assert crp[-1] == 0                   # a chunk wholly at or below the diagonal holds no pair
        assert got == whole, cuts


# ---------------------------------------------------------------- duplicate_groups
def _components_bfs(pairs, n):
    adj = [[] for _ in range(n)]
    for i, j in pairs:
        adj[i].append(j)
        adj[j].append(i)
    group = [-1] * n
    for s in range(n):                                    # ascending: the first row to reach a component is its smallest
        if group[s] >= 0:
            continue
        group[s], queue = s, [s]
        while queue:
            u = queue.pop(0)
            for v in adj[u]:
                if group[v] < 0:
                    group[v] = s
                    queue.append(v)
    return np.array(group, np.int64)


def test_duplicate_groups_is_the_smallest_index_of_the_component():
    from ivit_amd.search import duplicate_groups
    rng = np.random.default_rng(0)
    for n, m in ((1, 0), (9, 0), (12, 5), (60, 25), (60, 200), (300, 150), (300, 280)):
        pairs = rng.integers(0, n, size=(m, 2))
        got = duplicate_groups(pairs, n)
        want = _components_bfs(pairs.tolist(), n)
        assert got.dtype == np.int64 and got.shape == (n,) and np.array_equal(got, want), (n, m)
        if m == 0:
            assert np.array_equal(got, np.arange(n))      # isolated rows are their own group
        assert (got <= np.arange(n)).all() and np.array_equal(got[got], got)
    n = 200                                               # one component spanning everything: a path in a shuffled order, the worst
    order = rng.permutation(n)                            # case for the number of rounds
    path = np.stack([order[:-1], order[1:]], 1)
    assert np.array_equal(duplicate_groups(path, n), np.zeros(n, np.int64))
    star = np.stack([np.full(n - 1, n - 1), np.arange(n - 1)], 1)
    assert np.array_equal(duplicate_groups(star, n), np.zeros(n, np.int64))
    mixed = np.array([[7, 3], [3, 7], [5, 5], [9, 8]])    # both orientations, a loop, isolated rows beside
    g = duplicate_groups(mixed, 11)
    assert g.tolist() == [0, 1, 2, 3, 4, 5, 6, 3, 8, 8, 10]
    assert (g == np.arange(11)).sum() == 9                # keep: one row per component
    with pytest.raises(ValueError):
        duplicate_groups(np.array([[0, 11]]), 11)
