"""Neighbour order statistics on the device (include/ivit_kth.h): every bit of kth and every above against the numpy statement
(`predict.kth_reference`), no tolerance anywhere.  The sweep crosses widths, row and query counts around the tile, wavefront and
workgroup, k on both sides of the old limit of 64, one part (one launch, no workspace) and several (the workspace form), both values;
then ties, signed zeros, values that differ in the last digit only, the old routes for k <= 64, the refusals and HDBSCAN at min_pts 70."""
import ctypes
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib, cluster  # noqa: E402
from ivit_amd.predict import hdbscan_reference, inv_norms_reference, kth_reference, kth_values_reference  # noqa: E402
from ivit_amd.search import Gallery  # noqa: E402
from test_density_gpu import blobs  # noqa: E402
from test_range_gpu import Guarded, H, P, _engine, dev  # noqa: E402,F401

_P = ctypes.c_void_p
SPLITS = (0, 1, 2, 3, 7)


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, np.float32).view(np.uint32)


def run_kth(H, q, x, w, qw, k, self_join=0, splits=0):
    """the entry by hand, the workspace and both outputs between guards -> (kth bits, above, bytes of workspace)"""
    d_x = dev(x)
    d_q, d_w, d_qw = d_x if self_join else dev(q), dev(w), dev(qw)
    nq, (rows, dim), n = d_q.shape[0], x.shape, ctypes.c_size_t()
    H.call("ivit_kth_workspace_bytes", nq, rows, dim, splits, self_join, ctypes.byref(n))
    ws, kth, above = Guarded(n.value), Guarded(4 * nq), Guarded(8 * nq)
    H.call("ivit_kth_similarity", P(d_q), nq, P(d_x), rows, dim, P(d_w), P(d_qw), k, self_join, splits, ws.ptr, n.value, kth.ptr, above.ptr)
    torch.cuda.synchronize()
    assert ws.guards_intact() and kth.guards_intact() and above.guards_intact(), "wrote outside an output"
    assert np.array_equal(d_x.cpu().numpy(), x) and np.array_equal(d_q.cpu().numpy(), x if self_join else q), "an input was written"
    return kth.payload().view(np.uint32).copy(), above.payload().view(np.int64).copy(), n.value


def check(H, q, x, w, qw, k, self_join, splits, what=None):
    got_kth, got_above, n = run_kth(H, q, x, w, qw, k, self_join, splits)
    kth, above = kth_reference(q, x, w, qw, k, bool(self_join))
    assert np.array_equal(got_kth, bits(kth)) and np.array_equal(got_above, above), (what, k, splits, np.flatnonzero(got_kth != bits(kth))[:4].tolist())
    return n, got_above


@pytest.mark.parametrize("self_join", [0, 1])
@pytest.mark.parametrize("cosine", [False, True])
@pytest.mark.parametrize("dim", [64, 192, 1024])          # KS = 1, 3 (prefetch), 16 (no prefetch)
def test_kth_sweep(H, dim, cosine, self_join):
    case, forms = 0, set()
    for rows in (1, 31, 33, 97, 300):
        x = blobs(rows, dim)
        w = inv_norms_reference(x) if cosine else None
        for nq in (rows,) if self_join else (1, 33, 129):
            q = x if self_join else blobs(nq, dim, seed=3)
            qw = inv_norms_reference(q) if cosine and not self_join else None
            for k in sorted({min(max(k, 1), rows) for k in (1, 2, 64, 65, rows // 2, rows)}):
                forms.add(check(H, q, x, w, qw, k, self_join, SPLITS[case % 5], (rows, nq))[0] > 0)
                case += 1
    assert forms == {False, True}                          # the one-launch form and the workspace form


@pytest.mark.parametrize("splits", [1, 3])
def test_kth_ties_signs_and_zero(H, splits):
    same = np.tile(blobs(1, 64), (97, 1))                  # everything ties: above == 0 whatever k
    for k in (1, 2, 65, 97):
        for self_join in (0, 1):
            assert not check(H, same if self_join else same[:33], same, None, None, k, self_join, splits, "ties")[1].any()
    x = blobs(40, 64, seed=1)
    x[7] = 0                                               # a row of zeros: its inverse norm is 0 and so is every value against it
    q = np.concatenate([x[:20], -x[20:]])                  # negative dots
    w, qw = inv_norms_reference(x), inv_norms_reference(q)
    w[9] = 0.0                                             # a weight of 0 on a row that is not: fl32(dot) * 0 is -0.0 under a negative dot
    v = kth_values_reference(q, x, w, qw, False)
    assert (v > 0).any() and (v < 0).any() and (v == 0).any() and (q.astype(np.int32) @ x[9].astype(np.int32) < 0).any()
    for k in range(1, 41):
        check(H, q, x, w, qw, k, 0, splits, "signs")
        check(H, x, x, w, None, k, 1, splits, "signs, self-join")


@pytest.mark.parametrize("splits", [0, 3])
def test_kth_values_that_differ_in_the_last_digit(H, splits):
    q = np.full((1, 1024), 127, np.int8)
    q[0, 0] = 1
    x = np.full((256, 1024), 65, np.int8)
    x[:, 0] = np.arange(256) - 128
    v = kth_values_reference(q, x, None, None, False)[0]
    assert np.array_equal(np.diff(v), np.ones(255, np.float32)) and 2 ** 23 <= v[0] and v[255] < 2 ** 24          # 256 consecutive integers
    assert len(set((v.view(np.uint32) >> 16).tolist())) == 1                               # the two leading digits agree throughout
    for k in (1, 2, 64, 65, 128, 191, 192, 193, 255, 256):
        check(H, q, x, None, None, k, 0, splits, "last digit")


@pytest.mark.parametrize("k", [1, 17, 64])
def test_kth_agrees_with_the_old_routes(k):
    x, q = blobs(300, 192, seed=9), blobs(33, 192, seed=4)
    for cosine in (False, True):
        kth, above = cluster.kth_similarity(dev(x), k, cosine=cosine, splits=3)
        assert np.array_equal(bits(kth), bits(cluster.core_similarity(dev(x), k, cosine=cosine))) and bool((above < k).all())
        gal = Gallery(dev(x), cosine=cosine)
        val = gal.search(dev(q), k)[1][:, k - 1] + 0.0
        assert np.array_equal(bits(gal.kth(dev(q), k, query_weight=None)[0]), bits(val))
    with pytest.raises(ValueError):
        Gallery(dev(x), chunk_rows=100).kth(dev(q), k)


def test_kth_refusals(H):
    """each refused before anything is launched: both outputs and the workspace keep their fill"""
    x, q, rows, dim = dev(blobs(97, 64)), dev(blobs(33, 64, seed=3)), 97, 64
    n, n33 = ctypes.c_size_t(), ctypes.c_size_t()
    H.call("ivit_kth_workspace_bytes", 97, rows, dim, 2, 0, ctypes.byref(n))
    H.call("ivit_kth_workspace_bytes", 33, rows, dim, 2, 0, ctypes.byref(n33))
    arena = Guarded(n.value + 16 * 97)
    ws = arena.ptr.value
    kth, above = ws + n.value + 8 * 97, ws + n.value
    INV, UNS, lib = _lib.IVIT_ERR_INVALID, _lib.IVIT_ERR_UNSUPPORTED, H.lib
    err = lambda: lib.ivit_last_error(H.h)                  # noqa: E731

    def call(q_=q.data_ptr(), nq=33, x_=x.data_ptr(), dim_=dim, k=5, self_join=0, bytes_=n.value, kth_=kth):
        return lib.ivit_kth_similarity(H.h, _P(q_), nq, _P(x_), rows, dim_, None, None, k, self_join, 2, _P(ws), bytes_, _P(kth_), _P(above))

    assert call(k=0) == INV and b"k must be" in err() and call(k=rows + 1) == INV and b"k must be" in err()
    assert call(dim_=96) == UNS and call(self_join=1) == INV and b"nq must equal rows" in err()
    assert call(q_=x.data_ptr() + 64, nq=97, self_join=1) == INV and b"q must be x" in err()
    assert 0 < n33.value < n.value and call(bytes_=n33.value - 1) == INV and b"workspace" in err()
    assert call(x_=x.data_ptr() + 4) == INV and b"x must be" in err() and call(kth_=kth + 2) == INV and b"kth must be" in err()
    assert call(kth_=x.data_ptr()) == INV and b"x and kth overlap" in err()
    assert call(kth_=above) == INV and b"overlap" in err() and call(kth_=None) == INV and b"null" in err()
    assert lib.ivit_kth_workspace_bytes(H.h, 33, rows, 96, 2, 0, ctypes.byref(n)) == UNS and lib.ivit_kth_workspace_bytes(H.h, 33, rows, dim, 2, 1, ctypes.byref(n)) == INV
    torch.cuda.synchronize()
    assert arena.untouched(), "a refused call wrote"
    assert call() == 0 and call(q_=x.data_ptr(), nq=97, self_join=1) == 0       # and the same arguments, unharmed, are accepted
    torch.cuda.synchronize()
    assert arena.guards_intact() and not arena.untouched()


@pytest.mark.parametrize("fname", ["micro_vit2h_b3.npz", "micro_swin_b2.npz"])
def test_engine_knn_novelty(fname):
    cfg, eng = _engine(fname)
    images = torch.from_numpy(iv.make_images_int8(cfg, 140, seed=31)).cuda()
    f8 = torch.cat([eng.features(images[i:i + 35], copy=True)[0] for i in range(0, 140, 35)])
    gal, x = Gallery(f8[9:]), f8[9:].cpu().numpy()
    score, feat8 = eng.knn_novelty(images[:9], gal, 70, copy=True)
    want = kth_reference(f8[:9].cpu().numpy(), x, inv_norms_reference(x), inv_norms_reference(f8[:9].cpu().numpy()), 70)[0]
    assert torch.equal(feat8, f8[:9]) and np.array_equal(bits(score), bits(want))


def test_hdbscan_with_min_pts_above_64():
    x = blobs(300, 64, seed=2)
    w = inv_norms_reference(x)
    want = hdbscan_reference(x, w, 70)
    assert np.array_equal(bits(want[0]), bits(kth_reference(x, x, w, None, 70, True)[0]))
    _, core, tree, _ = cluster.hdbscan(dev(x), 5, min_pts=70)
    got = [t.cpu().numpy() for t in (tree.u, tree.v, tree.val)]
    assert np.array_equal(bits(core), bits(want[0])) and np.array_equal(bits(cluster.core_similarity(dev(x), 70)), bits(want[0]))
    assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want[1:])) and np.array_equal(bits(got[2]), bits(want[3]))
