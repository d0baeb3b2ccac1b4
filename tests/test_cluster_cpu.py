"""Exact integer k-means without a GPU: include/ivit_cluster.h declares four entries under version 1 beside ten unchanged headers, the
binding follows it and the build its mtime; the numpy statements of predict.py against brute force and at the rounding's edges;
the host seeding; purity and NMI on hand tables; KMeansStats.all_reduce over two gloo ranks."""
import ctypes
import os
import re
import socket

import numpy as np
import pytest

from conftest import ROOT
import ivit_amd as iv
from ivit_amd import _abi, _lib
from ivit_amd import cluster as cl
from ivit_amd.predict import (kmeans_assign_reference, kmeans_norms_reference, kmeans_reference, kmeans_stats_reference,
                              kmeans_update_reference)
from test_search_cpu import _prototypes_digest
from test_views_cpu import OLDER_HEADERS as NINE_OLDER

ENTRIES = {"ivit_kmeans_norms": 5, "ivit_kmeans_assign": 9, "ivit_kmeans_accumulate": 11, "ivit_kmeans_update": 8}

# the ten older headers: prototype count, version and sha256 of their prototypes.  The first nine are those test_views_cpu.py pins;
# ivit_views.h's was computed with the same function on the parent commit
OLDER_HEADERS = dict(NINE_OLDER, **{"ivit_views.h": (3, 1, "2eefaa0da335ec1ad492caf4bc1284e69a343290af8676c9e7cbf20270964fec")})


# ---------------------------------------------------------------- the eleventh header and its binding
def test_cluster_header_declares_entries_and_version():
    hdr = open(os.path.join(ROOT, "include", "ivit_cluster.h")).read()
    assert re.search(r'#include "ivit\.h"', hdr)
    assert int(re.search(r"#define IVIT_CLUSTER_VERSION (\d+)", hdr).group(1)) == 1 == _lib.IVIT_CLUSTER_VERSION
    assert _abi.CLUSTER_ABI.constants == {"IVIT_CLUSTER_VERSION": 1}
    assert list(_abi.CLUSTER_ABI.functions) == list(ENTRIES)
    for name in ENTRIES:                                  # one "Alignment:" and one "Overlap:" line in front of every entry
        m = re.search(r"\bint %s\(" % name, hdr)
        front = hdr[hdr.rfind(";", 0, m.start()) + 1:m.start()]
        assert len(re.findall(r"\bAlignment:", front)) == 1 and len(re.findall(r"\bOverlap:", front)) == 1, name
    fns = _abi.CLUSTER_ABI.functions
    assert [p.name for p in fns["ivit_kmeans_norms"].params] == ["h", "cent", "K", "dim", "cnorm"]
    assert [p.name for p in fns["ivit_kmeans_assign"].params] == ["h", "x", "rows", "dim", "cent", "cnorm", "K", "assign", "dist2"]
    assert [p.name for p in fns["ivit_kmeans_accumulate"].params] == ["h", "x", "assign", "dist2", "rows", "dim", "K", "splits", "sum", "count", "inertia"]
    assert [p.name for p in fns["ivit_kmeans_update"].params] == ["h", "sum", "count", "K", "dim", "cent", "cnorm", "moved"]
    assert "monotonic" in hdr.lower()                     # the header says that the inertia need not fall


def test_cluster_entries_bound_and_exported_beside_unchanged_headers():
    iv.build()
    lib = _lib.load()
    P, I, L = _lib._P, _lib._I, ctypes.c_int64
    assert list(_lib.CLUSTER_SIGNATURES) == list(ENTRIES) == list(_lib.CLUSTER_RESTYPES)
    for name, nparams in ENTRIES.items():             # every bound name is exported, with the header's parameter count
        bound = getattr(lib, name)
        assert len(_lib.CLUSTER_SIGNATURES[name]) == nparams and bound.argtypes == _lib.CLUSTER_SIGNATURES[name] and bound.restype is I, name
    assert _lib.CLUSTER_SIGNATURES["ivit_kmeans_norms"] == [P, P, I, I, P]
    assert _lib.CLUSTER_SIGNATURES["ivit_kmeans_assign"] == [P, P, L, I, P, P, I, P, P]
    assert _lib.CLUSTER_SIGNATURES["ivit_kmeans_accumulate"] == [P, P, P, P, L, I, I, I, P, P, P]
    assert _lib.CLUSTER_SIGNATURES["ivit_kmeans_update"] == [P, P, P, I, I, P, P, P]
    versions = (_lib.IVIT_VERSION, _lib.IVIT_EVAL_VERSION, _lib.IVIT_FEATURES_VERSION, _lib.IVIT_ATTNMAP_VERSION, _lib.IVIT_CLASSMAP_VERSION,
                _lib.IVIT_HIDDEN_VERSION, _lib.IVIT_SEARCH_VERSION, _lib.IVIT_MODELFILE_VERSION, _lib.IVIT_PROBE_VERSION, _lib.IVIT_VIEWS_VERSION)
    abis = (_lib.ABI, _lib.EVAL_ABI, _lib.FEATURES_ABI, _lib.ATTNMAP_ABI, _lib.CLASSMAP_ABI, _lib.HIDDEN_ABI, _lib.SEARCH_ABI, _lib.MODELFILE_ABI,
            _lib.PROBE_ABI, _lib.VIEWS_ABI)
    assert len(OLDER_HEADERS) == 10 == len(abis)
    older = set()
    for (name, (count, version, digest)), abi, v in zip(OLDER_HEADERS.items(), abis, versions):
        assert len(abi.functions) == count and v == version and _prototypes_digest(abi) == digest, name
        text = open(os.path.join(ROOT, "include", name)).read()
        assert _prototypes_digest(_abi.parse(text) if name == "ivit.h" else _abi.parse(text, base=_lib.ABI)) == digest, name
        assert "ivit_kmeans" not in text, name
        older |= set(abi.functions)
    assert not set(ENTRIES) & older
    with pytest.raises(_abi.AbiError):                    # it names a handle of ivit.h: it parses only with ivit.h as its base
        _abi.parse(open(_abi.CLUSTER_HEADER).read())


def test_build_follows_the_cluster_header():
    so = iv.build()
    assert os.path.getmtime(so) >= os.path.getmtime(_abi.CLUSTER_HEADER)
    assert "ivit_cluster.h" in _lib.SOURCES and os.path.exists(os.path.join(ROOT, "i-vit_amd", "csrc", "ivit_cluster.h"))
    src = open(os.path.join(ROOT, "i-vit_amd", "_lib.py")).read()
    assert re.search(r"newest = max\(.*_abi\.VIEWS_HEADER, _abi\.CLUSTER_HEADER", src)
    hip = open(os.path.join(ROOT, "i-vit_amd", "csrc", "ivit_hip.hip")).read()
    assert '#include "ivit_cluster.h"' in hip


def test_cluster_assign_on_both_engines():
    import inspect
    from ivit_amd import dist as ivdist, predict
    from ivit_amd.engine import ViTEngine
    from ivit_amd.native import NativeEngine
    from ivit_amd.swin_engine import SwinEngine
    for cls in (NativeEngine, ViTEngine, SwinEngine):
        assert list(inspect.signature(cls.cluster_assign).parameters)[1:3] == ["images", "kmeans"], cls
    assert list(inspect.signature(predict.kmeans_fit).parameters) == ["engine", "batches", "K", "iters", "init", "generator", "transform"]
    assert callable(ivdist.kmeans_fit_sharded)


# ---------------------------------------------------------------- the numpy statements
def _brute(x, c):
    d = ((x.astype(np.int64)[:, None, :] - c.astype(np.int64)[None, :, :]) ** 2).sum(axis=2)
    a = np.argmin(d, axis=1)                              # the first of the smallest: the lowest index
    return a.astype(np.int32), d[np.arange(len(a)), a].astype(np.int32)


@pytest.mark.parametrize("seed", range(4))
def test_assign_reference_is_the_nearest_centroid_lowest_index_first(seed):
    rng = np.random.default_rng(seed)
    rows, dim, K = 57, 64, (1, 5, 33, 40)[seed]
    lim = (128, 3, 128, 2)[seed]                          # a small alphabet: many exact ties
    x = rng.integers(-lim, lim, size=(rows, dim)).astype(np.int8)
    c = rng.integers(-lim, lim, size=(K, dim)).astype(np.int8)
    if K >= 5:
        c[4] = c[1]                                       # duplicate centroids: the lower index wins
        x[3] = c[1]
    a, d = kmeans_assign_reference(x, c)
    wa, wd = _brute(x, c)
    assert a.dtype == np.int32 and d.dtype == np.int32 and np.array_equal(a, wa) and np.array_equal(d, wd)
    if K >= 5:
        assert a[3] == 1 and d[3] == 0
    assert np.array_equal(kmeans_norms_reference(c), (c.astype(np.int64) ** 2).sum(axis=1))


def test_assign_reference_at_the_scores_extreme():
    x, c = np.full((2, 1024), -128, np.int8), np.full((3, 1024), -128, np.int8)
    c[0, 0] = 127
    a, d = kmeans_assign_reference(x, c)
    assert a.tolist() == [1, 1] and d.tolist() == [0, 0] and kmeans_norms_reference(c)[1] == 2 ** 24


def test_update_reference_rounds_half_up_and_keeps_empty_clusters():
    cent = np.array([[5] * 64, [6] * 64, [7] * 64, [9] * 64, [-3] * 64, [4] * 64], np.int8)
    count = np.array([2, 2, 0, 7, 7, 1], np.int64)
    total = np.zeros((6, 64), np.int64)
    total[0], total[1], total[2], total[3], total[4], total[5] = -3, 3, 1000, -128 * 7, 127 * 7, 4
    new, cnorm, moved = kmeans_update_reference(total, count, cent)
    assert new.dtype == np.int8 and cnorm.dtype == np.int32
    assert (new[0] == -1).all() and (new[1] == 2).all()   # -1.5 -> -1 and 1.5 -> 2: half up
    assert (new[2] == 7).all()                            # count 0: kept, whatever the sums hold
    assert (new[3] == -128).all() and (new[4] == 127).all() and (new[5] == 4).all()
    assert moved == 4 and np.array_equal(cnorm, (new.astype(np.int64) ** 2).sum(axis=1))
    # against the rational definition, elementwise: floor(mean + 1/2)
    rng = np.random.default_rng(1)
    n = rng.integers(1, 50, size=8)
    s = np.stack([rng.integers(-128 * k, 127 * k + 1, size=64) for k in n]).astype(np.int64)
    got, _, _ = kmeans_update_reference(s, n, np.zeros((8, 64), np.int8))
    from fractions import Fraction
    import math
    assert all(int(got[j, c]) == math.floor(Fraction(int(s[j, c]), int(n[j])) + Fraction(1, 2)) for j in range(8) for c in range(64))


def test_stats_reference_ignores_out_of_range_and_chains():
    rng = np.random.default_rng(3)
    x = rng.integers(-128, 128, size=(40, 64)).astype(np.int8)
    a = rng.integers(0, 4, size=40).astype(np.int32)
    a[[2, 9]] = (-1, 4)
    d = rng.integers(0, 1000, size=40).astype(np.int32)
    total, count, inertia = kmeans_stats_reference(x, a, d, 4)
    keep = (a >= 0) & (a < 4)
    assert count.sum() == 38 and inertia == d[keep].sum() and np.array_equal(total.sum(axis=0), x[keep].astype(np.int64).sum(axis=0))
    assert kmeans_stats_reference(x, a, None, 4)[2] == 0
    cent0 = x[:4].copy()
    cent, assign, hist = kmeans_reference(x, cent0, 3)
    assert cent.dtype == np.int8 and assign.dtype == np.int32 and hist.dtype == np.int64 and hist.shape == (3,)
    one, a1, h1 = kmeans_reference(x, cent0, 1)
    assert h1[0] == hist[0] and np.array_equal(a1, kmeans_assign_reference(x, cent0)[0])


# ---------------------------------------------------------------- the seeding
@pytest.mark.parametrize("method", ["sample", "kmeans++"])
def test_init_is_deterministic_and_gives_distinct_rows(method):
    rng = np.random.default_rng(8)
    rows = rng.integers(-4, 4, size=(500, 64)).astype(np.int8)
    rows[100:200] = rows[0]                               # many duplicates of one row
    a = cl.init_centroids(rows, 20, method, np.random.default_rng(5))
    b = cl.init_centroids(rows, 20, method, np.random.default_rng(5))
    c = cl.init_centroids(rows, 20, method, np.random.default_rng(6))
    assert a.dtype == np.int8 and a.shape == (20, 64) and np.array_equal(a, b) and not np.array_equal(a, c)
    assert len(np.unique(a, axis=0)) == 20
    assert all((rows == r).all(axis=1).any() for r in a)  # rows of the data
    small = cl.init_centroids(rows, 20, method, np.random.default_rng(5), init_rows=64)
    assert len(np.unique(small, axis=0)) == 20
    with pytest.raises(ValueError, match="distinct"):
        cl.init_centroids(np.repeat(rows[:3], 10, axis=0), 4, method, np.random.default_rng(0))
    with pytest.raises(ValueError):
        cl.init_centroids(rows, 4, "random", np.random.default_rng(0))


# ---------------------------------------------------------------- purity and NMI
def test_purity_and_nmi_on_hand_tables():
    perfect = np.array([[5, 0], [0, 7]])
    assert cl.purity(perfect) == 1.0 and abs(cl.nmi(perfect) - 1.0) < 1e-12
    indep = np.array([[2, 2], [2, 2]])
    assert cl.purity(indep) == 0.5 and abs(cl.nmi(indep)) < 1e-12
    t = np.array([[3, 1], [1, 3]])
    assert cl.purity(t) == 0.75
    mi = 2 * (3 / 8) * np.log((3 / 8) / 0.25) + 2 * (1 / 8) * np.log((1 / 8) / 0.25)
    assert abs(cl.nmi(t) - mi / np.log(2)) < 1e-12
    assert cl.nmi(np.array([[4]])) == 1.0 and np.isnan(cl.nmi(np.zeros((2, 2)))) and np.isnan(cl.purity(np.zeros((2, 2))))
    a, l = np.array([0, 0, 1, 1, 1, 5, -1]), np.array([0, 1, 1, 1, 0, 0, 1])
    want = np.array([[1, 1], [1, 2]])
    assert np.array_equal(cl.contingency_reference(a, l, 2, 2), want)
    import torch
    got = cl.contingency(torch.from_numpy(a), torch.from_numpy(l), 2, 2)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want)


# ---------------------------------------------------------------- two gloo ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _case():
    rng = np.random.default_rng(21)
    x = rng.integers(-128, 128, size=(101, 64)).astype(np.int8)
    cent = x[:6].copy()
    return x, cent


def _stats_worker(rank, world, port, q):
    import torch.distributed as dist
    from ivit_amd.dist import shard_range
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    x, cent = _case()
    lo, hi = shard_range(len(x), rank, world)
    a, d = kmeans_assign_reference(x[lo:hi], cent)
    stats = cl.KMeansStats.from_numpy(*kmeans_stats_reference(x[lo:hi], a, d, len(cent))).all_reduce()
    s, c, i = stats.numpy()
    q.put((rank, s.tobytes(), c.tobytes(), int(i)))
    dist.barrier()
    dist.destroy_process_group()


def test_kmeans_stats_all_reduce_world2_equals_one_rank():
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_stats_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    x, cent = _case()
    a, d = kmeans_assign_reference(x, cent)
    s, c, i = kmeans_stats_reference(x, a, d, len(cent))
    for rank, gs, gc, gi in res:
        assert gs == s.tobytes() and gc == c.tobytes() and gi == int(i), rank
