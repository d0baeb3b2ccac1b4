"""HDBSCAN without a GPU: include/ivit_hdbscan.h declares three entries under version 1 and the binding follows it; the host tree
(`Linkage.condense` / `CondensedTree.select` on the edges of `predict.hdbscan_reference`) against the brute force on the dense matrix
(`predict.hdbscan_labels_reference`), labels and stabilities to the bit, where ties are the rule; one planted case."""
import numpy as np
import pytest
from ivit_amd import _abi, _lib
from ivit_amd.cluster import Linkage
from ivit_amd.predict import hdbscan_labels_reference, hdbscan_reference, inv_norms_reference, mutual_reachability_reference
from test_density_gpu import blobs, chains

RUN = ["comp", "done", "edge_u", "edge_v", "edge_val", "state"]


def test_hdbscan_header_declares_entries():
    scan = ["h", "x", "rows", "dim", "weight"]
    assert _lib.IVIT_HDBSCAN_VERSION == 1 and {n: [p.name for p in f.params] for n, f in _abi.HDBSCAN_ABI.functions.items()} == {
        "ivit_core_workspace_bytes": ["h", "rows", "dim", "min_pts", "splits", "bytes"],
        "ivit_core_similarity": scan + ["min_pts", "splits", "workspace", "bytes", "core"],
        "ivit_reach_round": scan + ["core", "floor", "splits", "workspace", "bytes"] + RUN}
    hdr = open(_abi.HDBSCAN_HEADER).read()
    assert hdr.count("Alignment:") - 1 == hdr.count("Overlap:") - 1 == 3          # one pair per entry, and the convention's mention
    assert all(hasattr(_lib.load(), n) for n in _abi.HDBSCAN_ABI.functions)


def data(kind):
    if kind == "blobs":
        x = blobs(100, 64)
        return x, inv_norms_reference(x)
    if kind == "chains":                                   # shuffled chains: almost every value ties
        return chains(63, 20, seed=3)[0], None
    return np.tile(blobs(1, 64), (40, 1)), None            # all rows identical: ONE level


@pytest.mark.parametrize("min_pts", [1, 3, 5])
@pytest.mark.parametrize("mcs", [2, 5])
@pytest.mark.parametrize("kind", ["blobs", "chains", "identical"])
def test_host_tree_is_the_brute_force(kind, mcs, min_pts):
    x, w = data(kind)
    rows = x.shape[0]
    core, m = mutual_reachability_reference(x, w, min_pts)
    values = np.sort(m[np.triu_indices(rows, 1)])
    for floor in (None, values[(len(values) * 9) // 10]):
        _, u, v, val = hdbscan_reference(x, w, min_pts, floor)
        tree = Linkage(u, v, val, rows).condense(mcs, floor)
        for selection in ("eom", "leaf"):
            for single in (False, True):
                want, stability = hdbscan_labels_reference(m, mcs, floor, selection, single)
                got = tree.select(selection, single)
                assert got.dtype == want.dtype and np.array_equal(got, want), (floor, selection, single)
        assert {(int(n), float(b)): float(s) for n, b, s in zip(tree.name, tree.birth, tree.stability)} == stability, floor
    if kind == "identical":                                # one level: the root ends at its birth and is the only cluster
        assert len(tree.birth) == 1 and (tree.select("eom", True) == 0).all() and (tree.select("eom") == -1).all()


def test_planted_blobs_and_scattered_rows():
    """two tight blobs of 12 rows and 10 scattered rows: the labels are the planted groups, the scattered rows noise — asserted of the
    REFERENCE alone first: at least two clusters and some noise"""
    rng = np.random.default_rng(5)
    centre = rng.integers(-60, 61, size=(2, 64))
    centre[1, :32] = centre[0, :32]                        # a cosine near 0.5 between the blobs: they part above every scattered row
    x = np.concatenate([centre[0] + rng.integers(-2, 3, size=(12, 64)), centre[1] + rng.integers(-2, 3, size=(12, 64)),
                        rng.integers(-60, 61, size=(10, 64))]).astype(np.int8)
    order = rng.permutation(34)
    x, planted = x[order], np.repeat([0, 1, -1], [12, 12, 10])[order]
    w = inv_norms_reference(x)
    core, m = mutual_reachability_reference(x, w, 5)
    want, _ = hdbscan_labels_reference(m, 5)
    assert len(np.unique(want[want >= 0])) >= 2 and (want < 0).any()
    names = np.where(planted >= 0, [int(np.flatnonzero(planted == p).min()) for p in planted], -1)
    assert np.array_equal(want, names)
    _, u, v, val = hdbscan_reference(x, w, 5)
    assert np.array_equal(Linkage(u, v, val, 34).condense(5).select(), want)


# ---------------------------------------------------------------- the kernels in the code object
def test_core_kernels_in_code_object_without_scratch(tmp_path):
    from test_search_cpu import check_scan_kernels_in_code_object
    check_scan_kernels_in_code_object(tmp_path, "core_scan_kernel", [""])                                # the candidate slots are dynamic LDS
