"""Exact integer k-means on the device (include/ivit_cluster.h).  Everything is bit-exact against the numpy statements of
ivit_amd/predict.py (kmeans_assign_reference, kmeans_stats_reference, kmeans_update_reference, kmeans_reference): array_equal, no
tolerance anywhere, and nothing asserts that the inertia falls.

The assign sweep crosses widths (every regime of the register-resident rows and both sides of the prefetch boundary at 512), centroid
counts (one, a partial tile, one tile, one over, several tiles with a partial last) and row counts (one, partial and whole
wavefronts, partial and whole workgroups, several workgroups); planted ties, the last centroid, the score's extreme and zero distances;
both forms of the accumulate and every `splits`; the update in place with empty clusters; five chained iterations eager and replayed
from one graph; chunks; the engine; the refusals with every output between guard bands; one case beyond 2^31 bytes of rows."""
import ctypes

import numpy as np
import pytest

from conftest import golden_scales, load_golden
from large_cases import GIB, repeat_rows

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from ivit_amd import cluster as cl  # noqa: E402
from ivit_amd.predict import (kmeans_assign_reference, kmeans_norms_reference, kmeans_reference, kmeans_stats_reference,  # noqa: E402
                              kmeans_update_reference)

_P = ctypes.c_void_p
GUARD_BYTES = 4096
FILL = 0x5A
INV, UNS, OK = _lib.IVIT_ERR_INVALID, _lib.IVIT_ERR_UNSUPPORTED, _lib.IVIT_OK


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


def P(t):
    return None if t is None else _P(t.data_ptr())


def guarded(nbytes, fill=None):
    """(whole buffer, payload view): `nbytes` of payload between two 4 KiB guards filled with 0x5A; the payload zeroed, or holding
    the bytes of `fill`"""
    whole = torch.full((GUARD_BYTES + nbytes + GUARD_BYTES,), FILL, dtype=torch.uint8, device="cuda")
    pay = whole[GUARD_BYTES:GUARD_BYTES + nbytes]
    if fill is None:
        pay.zero_()
    else:
        pay.copy_(torch.from_numpy(np.ascontiguousarray(fill).view(np.uint8).reshape(-1)))
    return whole, pay


def guards_intact(whole, nbytes):
    return bool(((whole[:GUARD_BYTES] == FILL).all() & (whole[GUARD_BYTES + nbytes:] == FILL).all()).item())


def read(pay, dtype, shape=None):
    a = pay.cpu().numpy().view(dtype)
    return a if shape is None else a.reshape(shape)


def device_assign(H, x, cent, want_dist2=True, cnorm=None):
    """ivit_kmeans_norms + ivit_kmeans_assign of host arrays, every array between guard bands; the inputs must come back as they went"""
    rows, dim = x.shape
    K = cent.shape[0]
    xw, xd = guarded(rows * dim, x)
    cw, cd = guarded(K * dim, cent)
    nw, nd = guarded(4 * K)
    aw, ad = guarded(4 * rows)
    dw, dd = guarded(4 * rows)
    ad.fill_(0xEE)
    dd.fill_(0xEE)
    if cnorm is None:
        H.call("ivit_kmeans_norms", P(cd), K, dim, P(nd))
    else:
        nd.copy_(torch.from_numpy(cnorm.view(np.uint8)))
    H.call("ivit_kmeans_assign", P(xd), rows, dim, P(cd), P(nd), K, P(ad), P(dd) if want_dist2 else None)
    torch.cuda.synchronize()
    for w, p in ((xw, xd), (cw, cd), (nw, nd), (aw, ad), (dw, dd)):
        assert guards_intact(w, p.numel()), "wrote outside an array"
    assert np.array_equal(read(xd, np.int8, (rows, dim)), x) and np.array_equal(read(cd, np.int8, (K, dim)), cent)
    assert np.array_equal(read(nd, np.int32), kmeans_norms_reference(cent) if cnorm is None else cnorm)
    if not want_dist2:
        assert (dd == 0xEE).all().item()
    return read(ad, np.int32), read(dd, np.int32)


def same_assign(got, want, label):
    for name, g, w in zip(("assign", "dist2"), got, want):
        assert g.dtype == np.int32 and np.array_equal(g, w), (label, name, np.flatnonzero(g != w)[:6].tolist(), g[g != w][:6].tolist(), w[g != w][:6].tolist())


# ---------------------------------------------------------------- assign: the sweep
ROWS = (1, 31, 32, 33, 127, 128, 129, 1000)
KS = (1, 2, 31, 32, 33, 100, 1000)


@pytest.mark.parametrize("dim", [64, 192, 384, 512, 576, 1024])
def test_assign_sweep(H, dim):
    rng = np.random.default_rng(300 + dim)
    x = rng.integers(-128, 128, size=(1000, dim)).astype(np.int8)
    x[0, 0], x[-1, -1] = -128, -128
    # centroids near the rows (a row plus small noise) and far ones; a small alphabet in a third of the columns gives close calls
    cent = np.clip(x[rng.integers(0, 1000, size=1000)].astype(np.int32) + rng.integers(-2, 3, size=(1000, dim)), -128, 127).astype(np.int8)
    cent[::3] = rng.integers(-128, 128, size=cent[::3].shape).astype(np.int8)
    for K in KS:
        want = kmeans_assign_reference(x, cent[:K])           # a row's result depends on no other row: one reference per K
        for rows in ROWS:
            got = device_assign(H, x[:rows], cent[:K])
            same_assign(got, (want[0][:rows], want[1][:rows]), (dim, K, rows))
            assert got[0].min() >= 0 and got[0].max() < K
    got = device_assign(H, x[:129], cent[:33], want_dist2=False)  # a NULL dist2: assign alone
    assert np.array_equal(got[0], kmeans_assign_reference(x[:129], cent[:33])[0])


# ---------------------------------------------------------------- assign: planted cases
def test_assign_duplicate_centroids_lowest_index_wins(H):
    rng = np.random.default_rng(5)
    dim, K = 128, 100
    base = rng.integers(-100, 100, size=(K, dim)).astype(np.int8)
    for j in (0, 1, 3, 27, 30):                               # j, j + 4 (the other lane half), j + 32, j + 64 (other tiles)
        cent = base.copy()
        for o in (4, 32, 64):
            cent[j + o] = cent[j]
        x = np.repeat(cent[j][None, :], 40, axis=0)
        x[1::2, 0] = np.clip(x[1::2, 0].astype(np.int32) + 1, -128, 127)       # every second row one step away: still nearest to j
        got = device_assign(H, x, cent)
        same_assign(got, kmeans_assign_reference(x, cent), ("duplicates", j))
        assert (got[0] == j).all() and (got[1][0::2] == 0).all()
        for drop in (j, j + 4):                               # without the lower copies the next one wins
            cent[drop] = ~cent[drop]
            got = device_assign(H, x, cent)
            same_assign(got, kmeans_assign_reference(x, cent), ("duplicates", j, drop))
            assert (got[0] == drop + (4 if drop == j else 28)).all()


def test_assign_zero_row_against_centroids_of_equal_norm(H):
    dim, K = 64, 70
    rng = np.random.default_rng(6)
    cent = np.where(rng.integers(0, 2, size=(K, dim)) > 0, 3, -3).astype(np.int8)      # every norm 9 * 64
    x = np.zeros((5, dim), np.int8)
    got = device_assign(H, x, cent)
    assert (got[0] == 0).all() and (got[1] == 9 * dim).all()
    same_assign(got, kmeans_assign_reference(x, cent), "zero rows")


@pytest.mark.parametrize("K", [33, 45, 63, 95])
def test_assign_last_centroid_unique_winner_and_tied_loser(H, K):
    dim = 192
    rng = np.random.default_rng(K)
    cent = rng.integers(-128, 128, size=(K, dim)).astype(np.int8)
    x = np.repeat(cent[K - 1][None, :], 130, axis=0)          # the last centroid (K % 32 != 0) is the unique winner ...
    got = device_assign(H, x, cent)
    assert (got[0] == K - 1).all() and (got[1] == 0).all()
    same_assign(got, kmeans_assign_reference(x, cent), ("last wins", K))
    for j in (0, K - 2):                                      # ... and loses the tie against an equal centroid before it
        tied = cent.copy()
        tied[j] = tied[K - 1]
        got = device_assign(H, x, tied)
        assert (got[0] == j).all() and (got[1] == 0).all()
        same_assign(got, kmeans_assign_reference(x, tied), ("last loses", K, j))


def test_assign_every_byte_minus_128_at_dim_1024(H):
    dim, K = 1024, 40
    x = np.full((33, dim), -128, np.int8)
    cent = np.full((K, dim), -128, np.int8)
    cent[:7] = 127                                            # the most negative scores first
    cent[9, 5] = -127
    x[2] = 127                                                # and one row at the other end
    got = device_assign(H, x, cent)
    want = kmeans_assign_reference(x, cent)
    same_assign(got, want, "extreme")
    assert got[0][0] == 7 and got[1][0] == 0 and got[0][2] == 0 and got[1][2] == 0
    far = np.full((3, dim), 127, np.int8)                     # the largest distance: 255^2 * 1024 < 2^26
    got = device_assign(H, x[:2], far)
    assert (got[0] == 0).all() and (got[1] == 255 * 255 * 1024).all()


def test_assign_dist2_zero_where_a_row_equals_its_centroid(H):
    rng = np.random.default_rng(11)
    dim, K = 384, 50
    cent = rng.integers(-128, 128, size=(K, dim)).astype(np.int8)
    pick = rng.integers(0, K, size=200)
    x = cent[pick].copy()
    got = device_assign(H, x, cent)
    assert np.array_equal(got[0], pick) and not got[1].any()


# ---------------------------------------------------------------- accumulate
class Stats:
    """sum, count and inertia of a (K, dim), each between guard bands, holding `init` (default zeros)"""

    def __init__(self, K, dim, init=None):
        self.K, self.dim = K, dim
        self.sizes = (8 * K * dim, 8 * K, 8)
        init = init or (None, None, None)
        self.whole, self.pay = zip(*(guarded(n, f) for n, f in zip(self.sizes, init)))

    def ptrs(self):
        return tuple(P(p) for p in self.pay)

    def read(self):
        s, c, i = (read(p, np.int64) for p in self.pay)
        return s.reshape(self.K, self.dim), c, i[0]

    def intact(self):
        return all(guards_intact(w, n) for w, n in zip(self.whole, self.sizes))


def device_accumulate(H, x, a, d, K, splits, out):
    rows, dim = x.shape
    xw, xd = guarded(rows * dim, x)
    aw, ad = guarded(4 * rows, a)
    dw, dd = guarded(4 * rows, d) if d is not None else (None, None)
    ps = out.ptrs()
    H.call("ivit_kmeans_accumulate", P(xd), P(ad), P(dd), rows, dim, K, splits, *ps)
    torch.cuda.synchronize()
    assert out.intact() and guards_intact(xw, xd.numel()) and guards_intact(aw, ad.numel()), "wrote outside an array"
    assert np.array_equal(read(xd, np.int8, (rows, dim)), x) and np.array_equal(read(ad, np.int32), a)
    if d is not None:
        assert guards_intact(dw, dd.numel()) and np.array_equal(read(dd, np.int32), d)


def same_stats(got, want, label):
    for name, g, w in zip(("sum", "count", "inertia"), got, want):
        assert np.array_equal(np.asarray(g), np.asarray(w)), (label, name, np.argwhere(np.asarray(g) != np.asarray(w))[:4].tolist())


# (K, dim): the LDS copy where K (dim + 1) int32 fit 64 KB (84 x 193 words are 64 848 bytes, 85 x 193 are 65 620) and straight global adds
@pytest.mark.parametrize("K,dim,lds", [(10, 64, True), (84, 192, True), (85, 192, False), (1000, 64, False), (17, 1024, False)])
def test_accumulate_both_forms_every_split(H, K, dim, lds):
    assert (K * (dim + 1) * 4 <= 65536) == lds
    rng = np.random.default_rng(K + dim)
    rows = 777
    x = rng.integers(-128, 128, size=(rows, dim)).astype(np.int8)
    a = rng.integers(0, K, size=rows).astype(np.int32)
    a[[0, 5, 300, 776]] = (-1, K, -2 ** 31, 2 ** 31 - 1)     # ignored
    d = rng.integers(0, 2 ** 26 + 1, size=rows).astype(np.int32)
    want = kmeans_stats_reference(x, a, d, K)
    assert want[1].sum() == rows - 4
    first = None
    for splits in (0, 1, 2, 7):
        out = Stats(K, dim)
        device_accumulate(H, x, a, d, K, splits, out)
        same_stats(out.read(), want, (K, dim, splits))
        words = tuple(p.cpu().numpy().tobytes() for p in out.pay)
        first = first or words
        assert words == first                                 # the same words whatever the split
    # a NULL dist2 leaves the inertia untouched; the entry adds onto what the buffers hold
    init = (rng.integers(-2 ** 40, 2 ** 40, size=(K, dim)), rng.integers(0, 2 ** 40, size=K), np.array([12345678901], np.int64))
    out = Stats(K, dim, tuple(np.ascontiguousarray(t, np.int64) for t in init))
    device_accumulate(H, x, a, None, K, 0, out)
    same_stats(out.read(), (init[0] + want[0], init[1] + want[1], 12345678901), "NULL dist2 onto non-zero buffers")
    device_accumulate(H, x, a, d, K, 3, out)
    same_stats(out.read(), (init[0] + 2 * want[0], init[1] + 2 * want[1], 12345678901 + want[2]), "a second call")


def test_accumulate_beyond_one_flush_of_the_lds_copy(H):
    """70 001 rows of -128 in one part: more than the 65 536 rows between two flushes of the LDS copy"""
    rows, dim, K = 70001, 64, 2
    x = np.full((rows, dim), -128, np.int8)
    a = np.ones(rows, np.int32)
    d = np.full(rows, 2 ** 26, np.int32)
    out = Stats(K, dim)
    device_accumulate(H, x, a, d, K, 1, out)
    s, c, i = out.read()
    assert not s[0].any() and (s[1] == -128 * rows).all() and c.tolist() == [0, rows] and i == rows * 2 ** 26 > 2 ** 32


# ---------------------------------------------------------------- update
@pytest.mark.parametrize("K,dim", [(1, 64), (7, 192), (130, 1024)])
def test_update_in_place_against_the_reference(H, K, dim):
    rng = np.random.default_rng(K)
    cent = rng.integers(-128, 128, size=(K, dim)).astype(np.int8)
    count = rng.integers(1, 2 ** 33, size=K).astype(np.int64)
    count[::5] = rng.integers(1, 4, size=len(count[::5]))
    if K > 3:
        count[3] = 0                                          # an empty cluster keeps its centroid, whatever its sums hold
    mean = rng.integers(-128, 128, size=(K, dim)).astype(np.int64)
    total = mean * count[:, None] + rng.integers(0, 2, size=(K, dim)) * (count[:, None] // 2)       # many exact halves
    total = np.clip(total, -128 * count[:, None], 127 * count[:, None])
    if K > 3:
        total[3] = 99
    if K > 6:
        total[5], count[5] = -3, 2                            # -1.5 -> -1
        total[6], count[6] = 3, 2                             # 1.5 -> 2
        total[4] = cent[4].astype(np.int64) * count[4]        # the mean is the centroid: not moved
    new, cnorm, moved = kmeans_update_reference(total, count, cent)
    sw, sd = guarded(8 * K * dim, total)
    nw, nd = guarded(8 * K, count)
    cw, cd = guarded(K * dim, cent)
    qw, qd = guarded(4 * K)
    mw, md = guarded(8, np.array([1000], np.int64))           # added into, not written
    H.call("ivit_kmeans_update", P(sd), P(nd), K, dim, P(cd), P(qd), P(md))
    torch.cuda.synchronize()
    for w, p in ((sw, sd), (nw, nd), (cw, cd), (qw, qd), (mw, md)):
        assert guards_intact(w, p.numel())
    assert np.array_equal(read(sd, np.int64, (K, dim)), total) and np.array_equal(read(nd, np.int64), count)
    got = read(cd, np.int8, (K, dim))
    assert np.array_equal(got, new), np.argwhere(got != new)[:5].tolist()
    assert np.array_equal(read(qd, np.int32), cnorm) and read(md, np.int64)[0] == 1000 + moved
    if K > 6:
        assert (got[5] == -1).all() and (got[6] == 2).all() and np.array_equal(got[3], cent[3]) and np.array_equal(got[4], cent[4])
        assert moved <= K - 2


# ---------------------------------------------------------------- chained
def _blobs(rows=2000, dim=64, K=10, seed=17):
    rng = np.random.default_rng(seed)
    centres = rng.integers(-90, 91, size=(K, dim))
    x = np.clip(centres[rng.integers(0, K, size=rows)] + np.rint(rng.normal(0, 12, size=(rows, dim))), -128, 127).astype(np.int8)
    cent0 = cl.init_centroids(x, K, "kmeans++", np.random.default_rng(seed))
    return x, cent0


@pytest.fixture(scope="module")
def blobs():
    x, cent0 = _blobs()
    return x, cent0, kmeans_reference(x, cent0, 5), kmeans_reference(x, cent0, 10)


def test_fit_five_iterations_equals_the_reference(blobs):
    x, cent0, (cent, assign, hist), _ = blobs
    xd = torch.from_numpy(x).cuda()
    km = cl.KMeans(10, 64, "cuda:0").set_centroids(cent0)
    got = km.fit(xd, iters=5)
    assert got.dtype == np.int64 and np.array_equal(got, hist)
    c, n = km.numpy()
    assert np.array_equal(c, cent) and np.array_equal(n, kmeans_norms_reference(cent))
    assert np.array_equal(km.assign(xd)[0].cpu().numpy(), kmeans_assign_reference(x, cent)[0])
    # the assignment of the last iteration is what assign() gave against the centroids before the last update
    four = kmeans_reference(x, cent0, 4)[0]
    assert np.array_equal(kmeans_assign_reference(x, four)[0], assign)
    # tol_moved: one read per iteration, the loop ends once fewer than tol_moved centroids change; the history is a prefix
    km2 = cl.KMeans(10, 64, "cuda:0").set_centroids(cent0)
    early = km2.fit(xd, iters=5, tol_moved=11)
    assert len(early) == 1 and early[0] == hist[0] and km2.last_moved <= 10


def test_five_iterations_captured_in_one_graph(blobs):
    x, cent0, (cent, _, hist), (cent10, _, hist10) = blobs
    xd = torch.from_numpy(x).cuda()
    km = cl.KMeans(10, 64, "cuda:0")
    keep = torch.zeros(5, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    km.set_centroids(cent0)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):                           # eager once: the code is loaded and the buffers exist outside the capture
        km.step(xd)
    torch.cuda.synchronize()
    km.set_centroids(cent0)
    km.moved.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
        for i in range(5):
            km.step(xd)
            keep[i:i + 1].copy_(km.stats.inertia)
    torch.cuda.synchronize()
    assert np.array_equal(km.numpy()[0], cent0) and not keep.any().item()      # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(km.numpy()[0], cent) and np.array_equal(keep.cpu().numpy(), hist)
    graph.replay()                                            # five more, from where the first five ended
    torch.cuda.synchronize()
    assert np.array_equal(km.numpy()[0], cent10) and np.array_equal(keep.cpu().numpy(), hist10[5:])


def test_two_host_chunks_and_one_device_chunk_equal_the_single_tensor(blobs):
    x, cent0, (cent, _, hist), _ = blobs
    chunks = [torch.from_numpy(x[:700]), x[700:1301], torch.from_numpy(x[1301:]).cuda()]        # a host tensor, a numpy array, a device tensor
    km = cl.KMeans(10, 64, "cuda:0").set_centroids(cent0)
    got = km.fit(chunks, iters=5)
    assert np.array_equal(got, hist) and np.array_equal(km.numpy()[0], cent)


def test_contingency_on_the_device():
    rng = np.random.default_rng(2)
    a, l = rng.integers(-1, 8, size=500), rng.integers(0, 5, size=500)
    got = cl.contingency(torch.from_numpy(a).cuda(), torch.from_numpy(l).cuda(), 7, 5)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), cl.contingency_reference(a, l, 7, 5))


# ---------------------------------------------------------------- the engine
def test_engine_cluster_assign_equals_features_then_assign():
    from ivit_amd.engine import ViTEngine
    g = load_golden("micro_vit_b2.npz")
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    eng = ViTEngine.from_float(cfg, iv.make_vit_weights(cfg, int(g["seed"])), golden_scales(g))
    images = torch.from_numpy(iv.make_images_int8(cfg, 9, seed=3)).cuda()
    feat8 = eng.features(images, copy=True)[0]
    f8 = feat8.cpu().numpy()
    km = cl.KMeans(4, eng.num_features, eng.device).init(feat8, "sample", np.random.default_rng(1))
    want = tuple(t.clone() for t in km.assign(feat8))
    a, d, f = eng.cluster_assign(images, km, copy=True)
    assert torch.equal(a, want[0]) and torch.equal(d, want[1]) and torch.equal(f, feat8)
    ra, rd = kmeans_assign_reference(f8, km.numpy()[0])
    assert np.array_equal(a.cpu().numpy(), ra) and np.array_equal(d.cpu().numpy(), rd) and (rd == 0).sum() >= 4


def test_predict_kmeans_fit_equals_the_reference_on_the_engine_features():
    from ivit_amd import predict
    from ivit_amd.engine import ViTEngine
    g = load_golden("micro_vit_b2.npz")
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    eng = ViTEngine.from_float(cfg, iv.make_vit_weights(cfg, int(g["seed"])), golden_scales(g))
    batches = [torch.from_numpy(iv.make_images_int8(cfg, n, seed=s)).cuda() for n, s in ((5, 3), (4, 4))]
    f8 = torch.cat([eng.features(b, copy=True)[0] for b in batches]).cpu().numpy()
    km, feat8, hist = predict.kmeans_fit(eng, batches, K=3, iters=4, init="sample", generator=np.random.default_rng(5))
    assert feat8.dtype == torch.int8 and np.array_equal(feat8.cpu().numpy(), f8)
    cent0 = cl.init_centroids(f8, 3, "sample", np.random.default_rng(5))
    cent, _, want = kmeans_reference(f8, cent0, 4)
    assert np.array_equal(hist, want) and np.array_equal(km.numpy()[0], cent)


def test_kmeans_on_the_unindexed_device_takes_indexed_tensors_and_names_a_wrong_one(blobs):
    x, cent0, _, _ = blobs
    km = cl.KMeans(10, 64, "cuda").set_centroids(cent0)
    assert km.device == torch.device("cuda", torch.cuda.current_device())
    a, d = km.assign(torch.from_numpy(x[:100]).to("cuda:0"))
    ra, rd = kmeans_assign_reference(x[:100], cent0)
    assert np.array_equal(a.cpu().numpy(), ra) and np.array_equal(d.cpu().numpy(), rd)
    with pytest.raises(ValueError, match="on cuda:0"):
        km.assign(torch.from_numpy(x[:100]))
    with pytest.raises(ValueError, match="int8"):
        km.assign(torch.from_numpy(x[:100]).cuda().int())


# ---------------------------------------------------------------- the empty call and the refusals
def test_refusals_launch_nothing_and_name_the_argument(H):
    rng = np.random.default_rng(4)
    rows, dim, K = 70, 64, 6
    x = rng.integers(-128, 128, size=(rows, dim)).astype(np.int8)
    cent = x[:K].copy()
    a0, d0 = kmeans_assign_reference(x, cent)
    ins = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")  # the inputs far apart in ONE allocation
    xd = ins[:rows * dim].view(torch.int8).view(rows, dim)
    ad = ins[65536:65536 + 4 * rows].view(torch.int32)
    dd = ins[131072:131072 + 4 * rows].view(torch.int32)
    xd.copy_(torch.from_numpy(x))
    ad.copy_(torch.from_numpy(a0))
    dd.copy_(torch.from_numpy(d0))
    n_c, n_n, n_a, n_s, n_k = K * dim, 4 * K, 4 * rows, 8 * K * dim, 8 * K
    offs = np.cumsum([0, n_c, n_n + 8, n_a + 8, n_a, n_s, n_k, 8])       # cent, cnorm, assign, dist2, sum, count, inertia, moved
    whole, pay = guarded(int(offs[-1]) + 8)
    pay.fill_(FILL)
    cd, nd, oa, od, sm, ct, it, mv = (pay[int(o):int(o) + n] for o, n in zip(offs, (n_c, n_n, n_a, n_a, n_s, n_k, 8, 8)))
    assert all(t.data_ptr() % 8 == 0 for t in (cd, nd, oa, od, sm, ct, it, mv)) and cd.data_ptr() % 16 == 0
    lib, err = H.lib, lambda: H.lib.ivit_last_error(H.h)

    def norms(c=P(cd), K_=K, dim_=dim, n=P(nd)):
        return lib.ivit_kmeans_norms(H.h, c, K_, dim_, n)

    def assign(x_=P(xd), rows_=rows, dim_=dim, c=P(cd), n=P(nd), K_=K, a=P(oa), d=P(od)):
        return lib.ivit_kmeans_assign(H.h, x_, rows_, dim_, c, n, K_, a, d)

    def accumulate(x_=P(xd), a=P(ad), d=P(dd), rows_=rows, dim_=dim, K_=K, splits=0, s=P(sm), c=P(ct), i=P(it)):
        return lib.ivit_kmeans_accumulate(H.h, x_, a, d, rows_, dim_, K_, splits, s, c, i)

    def update(s=P(sm), c=P(ct), K_=K, dim_=dim, ce=P(cd), n=P(nd), m=P(mv)):
        return lib.ivit_kmeans_update(H.h, s, c, K_, dim_, ce, n, m)

    for fn in (norms, assign, accumulate, update):            # a bad dim or K
        for bad in (96, 0, 1088, 32):
            assert fn(dim_=bad) == UNS and b"dim" in err(), (fn.__name__, bad)
        for bad in (0, -1, 16385):
            assert fn(K_=bad) == INV and b"K" in err(), (fn.__name__, bad)
    assert assign(rows_=0) == OK and accumulate(rows_=0) == OK   # nothing to do: nothing launched
    assert assign(rows_=-1) == INV and accumulate(rows_=-1) == INV and b"rows" in err()
    assert assign(rows_=(2 ** 24 - 1) * 128 + 1) == UNS          # more rows than one launch holds
    assert accumulate(splits=-1) == INV and accumulate(splits=65536) == INV and b"splits" in err()
    for fn, nulls in ((norms, ("c", "n")), (assign, ("x_", "c", "n", "a")), (accumulate, ("x_", "a", "s", "c", "i")), (update, ("s", "c", "ce", "n", "m"))):
        for null in nulls:                                    # a null pointer
            assert fn(**{null: None}) == INV and b"null" in err(), (fn.__name__, null)
    # misalignment, named
    odd = lambda t, by: _P(t.data_ptr() + by)                 # noqa: E731
    for call, name in ((lambda: norms(c=odd(cd, 8)), b"cent"), (lambda: norms(n=odd(nd, 2)), b"cnorm"),
                       (lambda: assign(x_=odd(xd, 8), rows_=rows - 1), b"x"), (lambda: assign(c=odd(cd, 4), K_=K - 1), b"cent"),
                       (lambda: assign(a=odd(oa, 2)), b"assign"), (lambda: assign(d=odd(od, 1)), b"dist2"), (lambda: assign(n=odd(nd, 2)), b"cnorm"),
                       (lambda: accumulate(x_=odd(xd, 4), rows_=rows - 1), b"x"), (lambda: accumulate(a=odd(ad, 2)), b"assign"),
                       (lambda: accumulate(s=odd(sm, 4)), b"sum"), (lambda: accumulate(c=odd(ct, 4)), b"count"), (lambda: accumulate(i=odd(it, 4)), b"inertia"),
                       (lambda: update(ce=odd(cd, 8), K_=K - 1), b"cent"), (lambda: update(s=odd(sm, 4)), b"sum"), (lambda: update(m=odd(mv, 4)), b"moved"),
                       (lambda: update(n=odd(nd, 2)), b"cnorm")):
        assert call() == INV and b"aligned" in err() and name in err(), err()
    # an output over an input, and two outputs over each other: each overlap named
    pairs = [(lambda: norms(n=odd(cd, 16)), b"cent", b"cnorm"),
             (lambda: assign(a=P(xd)), b"x", b"assign"), (lambda: assign(d=odd(xd, 64)), b"x", b"dist2"), (lambda: assign(a=P(cd)), b"cent", b"assign"),
             (lambda: assign(d=P(nd)), b"cnorm", b"dist2"), (lambda: assign(d=odd(oa, n_a - 4)), b"assign", b"dist2"),
             (lambda: accumulate(s=P(xd)), b"x", b"sum"), (lambda: accumulate(c=P(ad)), b"assign", b"count"), (lambda: accumulate(i=odd(dd, 8)), b"dist2", b"inertia"),
             (lambda: accumulate(c=odd(sm, n_s - 8)), b"sum", b"count"), (lambda: accumulate(i=odd(sm, 8)), b"sum", b"inertia"),
             (lambda: accumulate(i=odd(ct, 8)), b"count", b"inertia"),
             (lambda: update(ce=odd(sm, 8)), b"sum", b"cent"), (lambda: update(n=P(ct)), b"count", b"cnorm"), (lambda: update(m=odd(sm, n_s - 8)), b"sum", b"moved"),
             (lambda: update(n=odd(cd, 16)), b"cent", b"cnorm"), (lambda: update(m=odd(cd, 8)), b"cent", b"moved"), (lambda: update(m=P(nd)), b"cnorm", b"moved")]
    for call, a, b in pairs:
        assert call() == INV, (a, b)
        e = err()
        assert b"overlap" in e and a in e and b in e, e
    torch.cuda.synchronize()
    assert np.all(whole.cpu().numpy() == FILL), "an empty or refused call wrote"
    assert np.array_equal(xd.cpu().numpy(), x) and np.array_equal(ad.cpu().numpy(), a0) and np.array_equal(dd.cpu().numpy(), d0)
    # and the same arguments, unharmed, are accepted: one whole iteration in these buffers
    cd.copy_(torch.from_numpy(cent.view(np.uint8).reshape(-1)))
    for t in (sm, ct, it, mv):
        t.zero_()
    assert norms() == OK and assign() == OK and accumulate(a=P(oa), d=P(od)) == OK and update() == OK, err()
    torch.cuda.synchronize()
    assert guards_intact(whole, pay.numel())
    assert np.array_equal(read(oa, np.int32), a0) and np.array_equal(read(od, np.int32), d0)
    want = kmeans_stats_reference(x, a0, d0, K)
    same_stats((read(sm, np.int64, (K, dim)), read(ct, np.int64), read(it, np.int64)[0]), want, "after the refusals")
    new, cnorm, moved = kmeans_update_reference(want[0], want[1], cent)
    assert np.array_equal(read(cd, np.int8, (K, dim)), new) and np.array_equal(read(nd, np.int32), cnorm) and read(mv, np.int64)[0] == moved


# ---------------------------------------------------------------- rows beyond 2^31 bytes
def test_assign_and_accumulate_with_row_offsets_beyond_2_31(H):
    """dim 1024, 2 097 153 rows: the last row begins at byte 2^31.  A block of 7 rows repeats; the last three rows are planted"""
    dim, rows, K = 1024, 2097153, 2
    assert (rows - 1) * dim == 2 ** 31
    need = rows * dim + 8 * rows + (1 << 28)
    free, _ = torch.cuda.mem_get_info()
    if free < need + GIB:
        pytest.skip(f"{free} bytes free on the device, {need} needed")
    rng = np.random.default_rng(31)
    cent = rng.integers(-128, 128, size=(K, dim)).astype(np.int8)
    block = cent[[0, 1, 1, 0, 1, 0, 0]].copy()
    block[:, 0] = np.arange(7) - 3                            # seven different rows, each still nearest to its centroid
    tail = cent[[1, 0, 1]].copy()
    tail[:, 1] = (50, -60, 70)
    ba, bd = kmeans_assign_reference(block, cent)
    ta, td = kmeans_assign_reference(tail, cent)
    assert ba.tolist() == [0, 1, 1, 0, 1, 0, 0] and ta.tolist() == [1, 0, 1] and len(set(bd.tolist())) > 3 and len(set(td.tolist())) == 3
    xd = repeat_rows(torch, torch.from_numpy(block).cuda(), rows)
    xd[rows - 3:] = torch.from_numpy(tail).cuda()
    want_a = repeat_rows(torch, torch.from_numpy(ba).cuda(), rows)
    want_d = repeat_rows(torch, torch.from_numpy(bd).cuda(), rows)
    want_a[rows - 3:] = torch.from_numpy(ta).cuda()
    want_d[rows - 3:] = torch.from_numpy(td).cuda()
    cd = torch.from_numpy(cent).cuda()
    nd = torch.from_numpy(kmeans_norms_reference(cent)).cuda()
    aw, ad = guarded(4 * rows)
    dw, dd = guarded(4 * rows)
    H.call("ivit_kmeans_assign", P(xd), rows, dim, P(cd), P(nd), K, P(ad), P(dd))
    torch.cuda.synchronize()
    assert guards_intact(aw, 4 * rows) and guards_intact(dw, 4 * rows)
    got_a, got_d = ad.view(torch.int32), dd.view(torch.int32)
    bad = torch.nonzero((got_a != want_a) | (got_d != want_d))
    assert bad.numel() == 0, (bad[:5].reshape(-1).tolist(), "2^31 bytes at row", rows - 1)
    assert got_a[rows - 3:].tolist() == [1, 0, 1] and got_d[rows - 3:].tolist() == td.tolist()
    out = Stats(K, dim)
    H.call("ivit_kmeans_accumulate", P(xd), P(ad), P(dd), rows, dim, K, 0, *out.ptrs())
    torch.cuda.synchronize()
    assert out.intact()
    s, c, i = out.read()
    full, rem = divmod(rows - 3, 7)
    body = np.concatenate([block[:rem], tail]).astype(np.int64)
    body_a = np.concatenate([ba[:rem], ta])
    want_s = np.stack([full * block[ba == j].astype(np.int64).sum(axis=0) + body[body_a == j].sum(axis=0) for j in range(K)])
    want_c = np.array([full * int((ba == j).sum()) + int((body_a == j).sum()) for j in range(K)], np.int64)
    want_i = full * int(bd.astype(np.int64).sum()) + int(bd[:rem].astype(np.int64).sum()) + int(td.astype(np.int64).sum())
    assert np.array_equal(s, want_s) and np.array_equal(c, want_c) and i == want_i
