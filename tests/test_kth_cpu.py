"""Neighbour order statistics without a GPU: include/ivit_kth.h declares two entries under version 1 and the binding follows it;
`predict.kth_reference` as a self-join is `mutual_reachability_reference`'s core wherever both apply; the kernels are in the gfx950
code object without scratch."""
import numpy as np
import pytest
from ivit_amd import _abi, _lib
from ivit_amd.predict import inv_norms_reference, kth_reference, mutual_reachability_reference
from test_density_gpu import blobs


def test_kth_header_declares_entries():
    assert _lib.IVIT_KTH_VERSION == 1 and {n: [p.name for p in f.params] for n, f in _abi.KTH_ABI.functions.items()} == {
        "ivit_kth_workspace_bytes": ["h", "nq", "rows", "dim", "splits", "self_join", "bytes"],
        "ivit_kth_similarity": ["h", "q", "nq", "x", "rows", "dim", "weight", "qweight", "k", "self_join", "splits", "workspace", "bytes", "kth",
                                "above"]}
    hdr = open(_abi.KTH_HEADER).read()
    assert hdr.count("Alignment:") - 1 == hdr.count("Overlap:") - 1 == 2          # one pair per entry, and the convention's mention
    assert list(_lib.KTH_SIGNATURES) == list(_abi.KTH_ABI.functions) and "ivit_kth.h" in _lib.SOURCES
    assert all(hasattr(_lib.load(), n) for n in _abi.KTH_ABI.functions)


@pytest.mark.parametrize("cosine", [False, True])
@pytest.mark.parametrize("k", [1, 2, 17, 64])
def test_kth_reference_self_join_is_the_core_similarity(k, cosine):
    x = blobs(97, 64)
    x[5] = 0                                               # a row of zeros: zeros of both signs before the fold
    w = inv_norms_reference(x) if cosine else None
    kth, above = kth_reference(x, x, w, None, k, self_join=True)
    core = mutual_reachability_reference(x, w, k)[0]
    assert kth.dtype == np.float32 and above.dtype == np.int64 and np.array_equal(kth.view(np.uint32), core.view(np.uint32))
    assert (above < k).all() and not (np.signbit(kth) & (kth == 0)).any()                  # never -0.0
    with pytest.raises(ValueError):
        kth_reference(x, x, w, None, 98, self_join=True)


def test_kth_kernels_in_code_object_without_scratch(tmp_path):
    from test_search_cpu import check_scan_kernels_in_code_object
    check_scan_kernels_in_code_object(tmp_path, "kth_scan_kernel", ["Lb0E", "Lb1E"])                     # the histograms are dynamic LDS
