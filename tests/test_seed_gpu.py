"""k-means++ seeding on the device (include/ivit_seed.h) against predict.kmeans_seed_reference, bit for bit: the shapes at which the scan
changes its path, fewer distinct rows than K, guard bytes round every array, a graph on a side stream, the refusals, KMeans.init."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from ivit_amd import _lib  # noqa: E402
from ivit_amd import cluster as cl  # noqa: E402
from ivit_amd.predict import kmeans_reference, kmeans_seed_reference  # noqa: E402

GUARD, FILL, PAT = 4096, 0x5A, 0xA5          # guard bytes and their fill; what every output holds before the call


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def guarded(nbytes, fill=None):
    whole = torch.full((2 * GUARD + nbytes,), FILL, dtype=torch.uint8, device="cuda")
    pay = whole[GUARD:GUARD + nbytes]
    pay.fill_(PAT) if fill is None else pay.copy_(torch.from_numpy(np.ascontiguousarray(fill).view(np.uint8).reshape(-1)))
    return whole, pay


def workspace_bytes(rows, dim, trials):
    n = ctypes.c_size_t(0)
    return _lib.load().ivit_kmeans_seed_workspace_bytes(rows, dim, trials, ctypes.byref(n)), n.value


def rows_of(rows, dim, seed=5):
    """blobs round a few centres clipped to int8, 20 copies of row 0 inside one part, one all-127 and one all-(-128) row"""
    rng = np.random.default_rng(seed)
    centres = rng.integers(-100, 100, size=(7, dim))
    x = np.clip(centres[rng.integers(7, size=rows)] + rng.integers(-30, 31, size=(rows, dim)), -128, 127).astype(np.int8)
    if rows > 40:
        x[5:25], x[rows // 2], x[rows - 2] = x[0], 127, -128
    return x


class Seeded:
    """one ivit_kmeans_seed over host arrays, every array between guard bands, every output pre-filled with PAT"""

    def __init__(self, H, x, K, first, draws, dim=None, trials=None, stream=None):
        rows, dim, trials = x.shape[0], dim or x.shape[1], trials or draws.shape[1]
        st, n = workspace_bytes(rows, x.shape[1], draws.shape[1])
        assert st == 0
        self.K, self.dim = K, x.shape[1]
        self.sizes = [x.size, draws.size * 8, n, K * x.shape[1], 4 * K, 4 * K, 8 * K, 4]
        self.bufs = [guarded(s, f) for s, f in zip(self.sizes, [x, draws] + [None] * 6)]
        self.args = (rows, dim, K, trials, first)
        self.H = H

    def call(self, **swap):
        p = {n: P(b[1]) for n, b in zip(("x", "draws", "ws", "cent", "cnorm", "idx", "potential", "picked"), self.bufs)}
        p.update(swap)
        return self.H.lib.ivit_kmeans_seed(self.H.h, p["x"], *self.args[:5], p["draws"], p["ws"], self.sizes[2], p["cent"], p["cnorm"], p["idx"],
                                           p["potential"], p["picked"])

    def outputs(self):
        torch.cuda.synchronize()
        assert all(bool(((w[:GUARD] == FILL).all() & (w[GUARD + s:] == FILL).all()).item()) for (w, _), s in zip(self.bufs, self.sizes)), "wrote outside an array"
        raw = [b[1].cpu().numpy() for b in self.bufs[3:]]
        return (raw[2].view(np.int32), raw[0].view(np.int8).reshape(self.K, self.dim), raw[1].view(np.int32), raw[3].view(np.int64), raw[4].view(np.int32))

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((b[1] == PAT).all().item()) for b in self.bufs[2:])


def same(got, want):
    picked = int(want[4][0])
    for g, w, name in zip(got, want, ("idx", "cent", "cnorm", "potential", "picked")):
        n = picked if name in ("cent", "cnorm") else len(w)
        assert g.dtype == w.dtype and np.array_equal(g[:n], w[:n]), name
    assert (got[1][picked:].view(np.uint8) == PAT).all() and (got[2][picked:].view(np.uint8) == PAT).all()     # left unwritten


# (rows, dim, K, trials): a single row; one row past a 32-row tile; one past a 256-row part at the last prefetching width; a full
# candidate tile at the first non-prefetching width; a ragged tail over many parts at the models' width; two load phases
@pytest.mark.parametrize("rows,dim,K,trials", [(1, 64, 1, 1), (33, 64, 2, 1), (129, 448, 9, 5), (257, 448, 9, 5), (1000, 512, 40, 32),
                                                 (4133, 384, 40, 5), (5000, 1024, 24, 8)])
def test_seed_equals_the_reference(H, rows, dim, K, trials):
    x = rows_of(rows, dim)
    first, draws = cl.seed_draws(rows, K, trials, np.random.default_rng(rows))
    want = kmeans_seed_reference(x, K, first, draws)
    assert want[4][0] == K and len(set(want[0].tolist())) == K
    s = Seeded(H, x, K, first, draws)
    assert s.call() == 0, H.lib.ivit_last_error(H.h)
    same(s.outputs(), want)
    assert np.array_equal(s.bufs[0][1].cpu().numpy().view(np.int8).reshape(x.shape), x)          # x is not written


def test_fewer_distinct_rows_than_K_stops_and_leaves_the_rest_unwritten(H):
    x = np.repeat(rows_of(5, 64, seed=9), 60, axis=0)            # 5 distinct rows, 300 rows: two parts
    first, draws = cl.seed_draws(300, 8, 3, np.random.default_rng(1))
    want = kmeans_seed_reference(x, 8, first, draws)
    assert want[4][0] == 5 and (want[0][5:] == -1).all() and want[3][4] == 0
    s = Seeded(H, x, 8, first, draws)
    assert s.call() == 0
    same(s.outputs(), want)


def test_seed_captured_on_a_side_stream_replays_to_the_eager_bytes(H):
    x = rows_of(700, 192)
    first, draws = cl.seed_draws(700, 6, 4, np.random.default_rng(3))
    s = Seeded(H, x, 6, first, draws)
    assert s.call() == 0
    eager = s.outputs()
    same(eager, kmeans_seed_reference(x, 6, first, draws))
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    H.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
            assert s.call() == 0
        for _ in range(3):
            for b in s.bufs[2:]:
                b[1].fill_(PAT)                                  # the workspace too: nothing is carried between calls
            torch.cuda.synchronize()
            graph.replay()
            assert all(np.array_equal(g, e) for g, e in zip(s.outputs(), eager))
    finally:
        H.set_stream(torch.cuda.current_stream().cuda_stream)


def test_refusals_launch_nothing(H):
    x = rows_of(64, 128)
    first, draws = cl.seed_draws(64, 4, 2, np.random.default_rng(0))
    INV, UNS = _lib.IVIT_ERR_INVALID, _lib.IVIT_ERR_UNSUPPORTED
    assert workspace_bytes(64, 96, 2)[0] == UNS and workspace_bytes(64, 128, 33)[0] == INV and workspace_bytes(0, 128, 2)[0] == INV
    for status, kw in ((UNS, dict(dim=96)), (INV, dict(trials=33)), (INV, dict(first=64))):
        s = Seeded(H, x, 4, kw.pop("first", first), draws, **kw)
        assert s.call() == status and s.untouched(), kw
    s = Seeded(H, x, 4, first, draws)
    assert s.call(idx=ctypes.c_void_p(s.bufs[0][1].data_ptr() + 16)) == INV and s.untouched()
    err = H.lib.ivit_last_error(H.h).decode()
    assert "overlap" in err and "idx" in err and "x" in err
    assert np.array_equal(s.bufs[0][1].cpu().numpy().view(np.int8).reshape(x.shape), x)


def test_init_on_the_device_then_fit_equals_the_reference_from_the_reference_seeds():
    x = rows_of(3000, 64, seed=2)
    xd = torch.from_numpy(x).cuda()
    km = cl.KMeans(12, 64, "cuda:0").init([xd[:1000], xd[1000:]], where="device", generator=np.random.default_rng(4))
    first, draws = cl.seed_draws(3000, 12, cl.default_trials(12), np.random.default_rng(4))
    idx, cent0, cnorm, _, _ = kmeans_seed_reference(x, 12, first, draws)
    assert np.array_equal(km.numpy()[0], cent0) and np.array_equal(km.numpy()[1], cnorm)
    got = cl.seed(xd, 12, generator=np.random.default_rng(4))
    assert np.array_equal(got[0].cpu().numpy(), idx) and np.array_equal(got[1].cpu().numpy(), cent0)
    hist = km.fit(xd, iters=2)
    cent, _, want = kmeans_reference(x, cent0, 2)
    assert np.array_equal(km.numpy()[0], cent) and np.array_equal(hist, want)
    with pytest.raises(ValueError, match="distinct"):
        cl.KMeans(8, 64, "cuda:0").init(torch.from_numpy(np.repeat(x[:5], 10, axis=0)).cuda(), where="device")
