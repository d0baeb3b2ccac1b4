"""Gallery search on the device (include/ivit_search.h).  Everything is bit-exact against the numpy statements
(`predict.search_reference`, `predict.inv_norms_reference`): array_equal on idx and on the BITS of val, no tolerance anywhere.

The sweep crosses query counts, gallery sizes (one row per rank, a partial tile, a tile boundary, several tiles), widths, k, the
number of parts (0 = the library's choice, forced counts, and one above rows / k so that some part holds fewer than k rows), both
weights and both ends of index_base.  Full-range int8 values give no equal neighbours (the arithmetic); values from [-3, 3] at
width 64 give many (the order): one row repeated, 8 rows tiled 512 times, weights of +0.0 and -0.0.  A gallery sorted ascending by
its score for query 0 makes every row pass the threshold filter (the compaction path at its worst), one sorted descending nothing
behind the first k; with 7 parts the best k rows lie all in the last part, or all in the first.  Then ivit_gallery_inv_norms,
ivit_search_merge, the refusals (outputs and their guards untouched), the engines end to end and a hipGraph replay."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import golden_scales, load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from ivit_amd.predict import embed8, inv_norms_reference, knn_evaluate, search_reference  # noqa: E402
from ivit_amd.search import Gallery, knn_classify, knn_reference, query_inv_norms  # noqa: E402

_P = ctypes.c_void_p
GUARD_BYTES = 4096
FILL = 0x5A
TOP = 2 ** 31 - 1


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


def P(t):
    return None if t is None else _P(t.data_ptr())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def guarded(nbytes):
    """(whole buffer, payload view): `nbytes` of payload between two 4 KiB guards, everything filled with 0x5A"""
    whole = torch.full((GUARD_BYTES + nbytes + GUARD_BYTES,), FILL, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD_BYTES:GUARD_BYTES + nbytes]


def guards_intact(whole, nbytes):
    w = whole.cpu().numpy()
    return bool(np.all(w[:GUARD_BYTES] == FILL) and np.all(w[GUARD_BYTES + nbytes:] == FILL))


def workspace_bytes(H, nq, rows, dim, k, splits):
    n = ctypes.c_size_t()
    H.call("ivit_search_workspace_bytes", nq, rows, dim, k, splits, ctypes.byref(n))
    return n.value


def run_search(H, d_q, d_g, d_w, k, base=0, splits=0, with_val=True):
    """ivit_search_topk on device arrays -> (idx int32 [nq, k], val bits uint32 [nq, k] or None); the guards around idx, val and
    the workspace must stay what they were"""
    (nq, dim), rows = d_q.shape, d_g.shape[0]
    nws = workspace_bytes(H, nq, rows, dim, k, splits)
    assert nws % (8 * nq * k) == 0 and (splits == 0 or nws == 8 * nq * k * splits)
    ws_all, ws = guarded(nws)
    idx_all, idx = guarded(4 * nq * k)
    val_all, val = guarded(4 * nq * k)
    H.call("ivit_search_topk", P(d_q), nq, P(d_g), rows, dim, P(d_w), k, base, splits, P(ws), nws, P(idx), P(val) if with_val else None)
    torch.cuda.synchronize()
    assert guards_intact(ws_all, nws) and guards_intact(idx_all, 4 * nq * k) and guards_intact(val_all, 4 * nq * k), "wrote outside an output"
    v = val.cpu().numpy().view(np.uint32).reshape(nq, k)
    if not with_val:
        assert np.all(val.cpu().numpy() == FILL)
    return idx.cpu().numpy().view(np.int32).reshape(nq, k), v if with_val else None


class Case:
    """a query set and a gallery on the host and on the device, with the gallery's inverse norms and the reference for the largest k
    asked of it: a smaller k is its first columns (the order is total), so ONE reference serves every k"""

    def __init__(self, q, g):
        self.q, self.g = q, g
        self.w = inv_norms_reference(g)
        self.d_q, self.d_g, self.d_w = dev(q), dev(g), dev(self.w)
        self._ref = {}

    def reference(self, weighted, k):
        kmax = min(64, self.g.shape[0])
        if weighted not in self._ref:
            self._ref[weighted] = search_reference(self.q, self.g, self.w if weighted else None, kmax)
        idx, val = self._ref[weighted]
        return idx[:, :k], bits(val)[:, :k]

    def check(self, H, k, weighted, base=0, splits=0, what=""):
        ri, rv = self.reference(weighted, k)
        gi, gv = run_search(H, self.d_q, self.d_g, self.d_w if weighted else None, k, base, splits)
        label = (what, self.q.shape, self.g.shape, k, weighted, base, splits)
        assert np.array_equal(gi.astype(np.int64) - base, ri), (label, "idx", np.argwhere(gi.astype(np.int64) - base != ri)[:4].tolist())
        assert np.array_equal(gv, rv), (label, "val", np.argwhere(gv != rv)[:4].tolist())


@functools.lru_cache(maxsize=None)
def random_case(nq, rows, dim, lo=-128, hi=128):
    rng = np.random.default_rng(1000003 * nq + 1009 * rows + dim + (0 if lo == -128 else 7))
    return Case(rng.integers(lo, hi, size=(nq, dim), dtype=np.int64).astype(np.int8),
                rng.integers(lo, hi, size=(rows, dim), dtype=np.int64).astype(np.int8))


# ---------------------------------------------------------------- the sweep
NQ = [1, 5, 67, 130]            # one query, a partial wavefront, a second and third wavefront, a second workgroup
ROWS = [None, 63, 64, 65, 1000, 4099]       # None: k rows, one per rank


@pytest.mark.parametrize("k", [1, 7, 16, 17, 64])
@pytest.mark.parametrize("dim", [64, 192, 1024])
def test_search_sweep(H, dim, k):
    for nq in NQ:
        for rows in ROWS:
            rows = k if rows is None else rows
            if k > rows:
                continue                                       # refused: test_search_refusals
            case = random_case(nq, rows, dim)
            for splits in (0, 1, 2, 7, rows // k + 1):          # the last: some part holds fewer than k rows
                for weighted in (False, True):
                    for base in (0, TOP - rows):
                        case.check(H, k, weighted, base, splits)


def test_search_without_val(H):
    case = random_case(5, 1000, 64)
    gi, gv = run_search(H, case.d_q, case.d_g, case.d_w, 7, with_val=False)
    assert gv is None and np.array_equal(gi, case.reference(True, 7)[0])


# ---------------------------------------------------------------- the order: equal neighbours
def equal_neighbours(vbits):
    """adjacent equal values in the ranked lists (the value of +0.0 and -0.0 taken as one)"""
    v = vbits.view(np.float32) + np.float32(0.0)
    return int((v[:, 1:] == v[:, :-1]).sum())


def test_search_small_range_values_tie(H):
    """int8 values from [-3, 3] at width 64: many equal neighbours by dot product and some by cosine; the full range gives none"""
    small, full = random_case(5, 4099, 64, -3, 4), random_case(5, 4099, 64)
    assert equal_neighbours(small.reference(False, 64)[1]) > 50 and equal_neighbours(small.reference(True, 64)[1]) > 0
    assert equal_neighbours(full.reference(False, 64)[1]) == 0 and equal_neighbours(full.reference(True, 64)[1]) == 0
    for k in (1, 16, 17, 64):
        for splits in (0, 1, 2, 7, 4099 // k + 1):
            for weighted in (False, True):
                small.check(H, k, weighted, 0, splits, "small range")
    small.check(H, 64, False, TOP - 4099, 7, "small range, top of the index range")


@pytest.mark.parametrize("rows", [64, 2000])
def test_search_one_row_repeated(H, rows):
    """every score of a query is the same: idx is index_base + 0 .. k - 1 for every number of parts"""
    rng = np.random.default_rng(3)
    g = np.repeat(rng.integers(-128, 128, size=(1, 64), dtype=np.int64).astype(np.int8), rows, axis=0)
    case = Case(rng.integers(-128, 128, size=(5, 64), dtype=np.int64).astype(np.int8), g)
    for k in (1, 16, 64):
        for splits in (0, 1, 2, 7, rows // k + 1):
            for weighted in (False, True):
                for base in (0, 12345):
                    gi, gv = run_search(H, case.d_q, case.d_g, case.d_w if weighted else None, k, base, splits)
                    assert np.array_equal(gi, np.tile(base + np.arange(k, dtype=np.int32), (5, 1))), (k, splits, weighted, base)
                    case.check(H, k, weighted, base, splits, "one row repeated")


def test_search_eight_rows_tiled(H):
    rng = np.random.default_rng(4)
    g = np.tile(rng.integers(-128, 128, size=(8, 64), dtype=np.int64).astype(np.int8), (512, 1))
    case = Case(rng.integers(-128, 128, size=(5, 64), dtype=np.int64).astype(np.int8), g)
    assert equal_neighbours(case.reference(False, 64)[1]) == 5 * 63
    for k in (7, 16, 64):
        for splits in (0, 1, 2, 7, 4096 // k + 1):
            for weighted in (False, True):
                case.check(H, k, weighted, 0, splits, "8 rows tiled 512 times")


def test_search_signed_zero_weights(H):
    """weights of +0.0 and -0.0 against positive and negative dot products: +0.0 and -0.0 values tie, the index decides, and val
    keeps the sign"""
    rng = np.random.default_rng(6)
    q = rng.integers(-128, 128, size=(5, 64), dtype=np.int64).astype(np.int8)
    g = rng.integers(-128, 128, size=(1000, 64), dtype=np.int64).astype(np.int8)
    w = np.where(np.arange(1000) % 2 == 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    w[::200] = np.float32(-0.25)                                # ten rows with a value, negative weights among them: a few positive
    w[100::200] = np.float32(0.5)                               # values lead, then the zeros of both signs by index
    d_q, d_g, d_w = dev(q), dev(g), dev(w)
    for k in (16, 64):
        ri, rv = search_reference(q, g, w, k)
        assert (bits(rv) == 0x80000000).any() and (bits(rv) == 0).any()
        for splits in (0, 1, 7, 1000 // k + 1):
            gi, gv = run_search(H, d_q, d_g, d_w, k, 0, splits)
            assert np.array_equal(gi, ri) and np.array_equal(gv, bits(rv)), (k, splits)
    w0 = np.where(np.arange(1000) % 3 == 0, np.float32(-0.0), np.float32(0.0)).astype(np.float32)       # nothing but zeros
    ri, rv = search_reference(q, g, w0, 64)
    assert np.array_equal(ri, np.tile(np.arange(64, dtype=np.int32), (5, 1)))
    for splits in (0, 2, 7):
        gi, gv = run_search(H, d_q, d_g, dev(w0), 64, 0, splits)
        assert np.array_equal(gi, ri) and np.array_equal(gv, bits(rv))


# ---------------------------------------------------------------- the adversarial orders for a threshold filter
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ascending", [True, False])
def test_search_gallery_sorted_by_score(H, ascending, weighted):
    """ascending: every row beats query 0's threshold, every tile ends in a compaction; descending: nothing passes behind the first
    k.  With 7 parts the best k rows lie all in the last part, or all in the first."""
    base = random_case(5, 4099, 64)
    v = (base.q[:1].astype(np.int32) @ base.g.astype(np.int32).T).astype(np.float32)[0]
    if weighted:
        v = v * base.w
    order = np.argsort(v if ascending else -v, kind="stable")
    case = Case(base.q, base.g[order])
    ri, _ = case.reference(weighted, 64)
    part = -(-4099 // 7)
    assert np.all(ri[0] // part == (6 if ascending else 0))     # query 0's best 64 rows: all in the last / the first of 7 parts
    for k in (16, 64):
        for splits in (0, 1, 2, 7):
            case.check(H, k, weighted, 0, splits, "ascending" if ascending else "descending")


# ---------------------------------------------------------------- ivit_gallery_inv_norms
@pytest.mark.parametrize("rows", [1, 63, 4099])
@pytest.mark.parametrize("dim", [16, 64, 192, 1024])
def test_gallery_inv_norms_every_bit(H, dim, rows):
    rng = np.random.default_rng(dim + rows)
    g = rng.integers(-128, 128, size=(rows, dim), dtype=np.int64).astype(np.int8)
    cases = [g, np.zeros_like(g), np.full_like(g, -128)]
    single = np.zeros_like(g)
    single[np.arange(rows), rng.integers(0, dim, size=rows)] = rng.choice(np.array([-128, -1, 1, 3, 127], np.int8), size=rows)
    mixed = g.copy()
    mixed[::3] = 0
    mixed[1::5] = -128
    for c in cases + [single, mixed]:
        d_g = dev(c)
        out_all, out = guarded(4 * rows)
        H.call("ivit_gallery_inv_norms", P(d_g), rows, dim, P(out))
        torch.cuda.synchronize()
        assert guards_intact(out_all, 4 * rows)
        got = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, bits(inv_norms_reference(c)))


def test_gallery_inv_norms_refusals(H):
    g = dev(np.ones((8, 64), np.int8))
    out_all, out = guarded(4 * 8)
    call = lambda *a: getattr(H.lib, "ivit_gallery_inv_norms")(H.h, *a)       # noqa: E731
    assert call(P(g), 8, 24, P(out)) == _lib.IVIT_ERR_UNSUPPORTED
    assert call(P(g), -1, 64, P(out)) == _lib.IVIT_ERR_INVALID
    assert call(_P(g.data_ptr() + 1), 7, 64, P(out)) == _lib.IVIT_ERR_INVALID
    assert call(P(g), 8, 64, _P(g.data_ptr() + 64)) == _lib.IVIT_ERR_INVALID and b"overlap" in H.lib.ivit_last_error(H.h)
    assert call(P(g), 0, 64, P(out)) == _lib.IVIT_OK
    torch.cuda.synchronize()
    assert np.all(out_all.cpu().numpy() == FILL)


# ---------------------------------------------------------------- ivit_search_merge
def run_merge(H, ci, cv, k):
    nq, ncand = ci.shape
    idx_all, idx = guarded(4 * nq * k)
    val_all, val = guarded(4 * nq * k)
    d_ci, d_cv = dev(ci), dev(cv)
    H.call("ivit_search_merge", P(d_ci), P(d_cv), nq, ncand, k, P(idx), P(val))
    torch.cuda.synchronize()
    assert guards_intact(idx_all, 4 * nq * k) and guards_intact(val_all, 4 * nq * k)
    return idx.cpu().numpy().view(np.int32).reshape(nq, k), val.cpu().numpy().view(np.uint32).reshape(nq, k)


def merge_reference(ci, cv, k):
    """the k best candidates of each row from (val, idx) alone: descending by value, -0.0 equal to +0.0, equal values by ascending idx"""
    order = np.stack([np.lexsort((i, -(v + np.float32(0.0))))[:k] for i, v in zip(ci, cv)])
    return np.take_along_axis(ci, order, 1), bits(np.take_along_axis(cv, order, 1))


@pytest.mark.parametrize("nq", [1, 67])
@pytest.mark.parametrize("weighted", [False, True])
def test_search_merge_of_chunks_equals_one_call(H, weighted, nq):
    for lo, hi in ((-128, 128), (-3, 4)):
        case = random_case(nq, 4099, 64, lo, hi)
        for k in (7, 64):
            ci, cv = [], []
            for a, b in ((0, 1000), (1000, 2000), (2000, 4099)):
                gi, gv = run_search(H, case.d_q, case.d_g[a:b], case.d_w[a:b] if weighted else None, k, a, 0)
                ci.append(gi)
                cv.append(gv.view(np.float32))
            ci, cv = np.concatenate(ci, 1), np.concatenate(cv, 1)
            mi, mv = run_merge(H, ci, cv, k)
            ri, rv = case.reference(weighted, k)
            assert np.array_equal(mi, ri) and np.array_equal(mv, rv), (lo, k)
            wi, wv = merge_reference(ci, cv, k)
            assert np.array_equal(mi, wi) and np.array_equal(mv, wv)
            si, sv = run_merge(H, ci[:, :k], cv[:, :k], k)      # ncand == k: the candidates, sorted (they were already)
            assert np.array_equal(si, ci[:, :k]) and np.array_equal(sv, bits(cv[:, :k]))


def test_search_merge_signed_zeros_and_shuffled_candidates(H):
    rng = np.random.default_rng(8)
    nq, ncand = 5, 300
    ci = np.stack([rng.permutation(100000)[:ncand] for _ in range(nq)]).astype(np.int32)
    ci[0, :3] = [TOP - 1, 0, 1]
    cv = rng.choice(np.array([0.0, -0.0, 1.5, -1.5, 2.0 ** -126, 3.0e38, -3.0e38], np.float32), size=(nq, ncand)).astype(np.float32)
    for k in (1, 16, 64):
        mi, mv = run_merge(H, ci, cv, k)
        wi, wv = merge_reference(ci, cv, k)
        assert np.array_equal(mi, wi) and np.array_equal(mv, wv), k
    mi, mv = run_merge(H, ci[:, :64], cv[:, :64], 64)           # ncand == k, unsorted: a full sort
    wi, wv = merge_reference(ci[:, :64], cv[:, :64], 64)
    assert np.array_equal(mi, wi) and np.array_equal(mv, wv)


def test_search_second_phase_paths(H):
    """the second phase holds a query's parts * k keys in registers up to 1024 (16 per lane) and up to 4096 (64 per lane) and rescans
    them from memory beyond: both sides of both thresholds, through the search and through the merge"""
    for lo, hi in ((-128, 128), (-3, 4)):
        case = random_case(5, 4099, 64, lo, hi)
        for k, parts in ((16, 64), (16, 65), (16, 256), (16, 257), (7, 146), (7, 147), (7, 585), (7, 586), (64, 16), (64, 17), (64, 64), (64, 65)):
            assert parts * k in (1024, 1040, 4096, 4112, 1022, 1029, 4095, 4102, 1088, 4160)
            for weighted in (False, True):
                case.check(H, k, weighted, 0, parts, "second phase")
    rng = np.random.default_rng(9)
    for ncand in (1024, 1025, 4096, 4097):
        ci = np.stack([rng.permutation(1 << 20)[:ncand] for _ in range(3)]).astype(np.int32)
        cv = rng.choice(np.array([0.0, -0.0, 1.5, -1.5, 7.25], np.float32), size=(3, ncand)).astype(np.float32)
        cv[:, ::3] = rng.standard_normal((3, len(range(0, ncand, 3)))).astype(np.float32)
        for k in (1, 17, 64):
            mi, mv = run_merge(H, ci, cv, k)
            wi, wv = merge_reference(ci, cv, k)
            assert np.array_equal(mi, wi) and np.array_equal(mv, wv), (ncand, k)


def test_gallery_in_chunks_equals_one_piece(H):
    """the Python class: a device tensor, chunk_rows, and a list of device and HOST chunks give the same (idx, val)"""
    case = random_case(67, 4099, 64, -3, 4)
    for cosine in (True, False):
        ri, rv = case.reference(cosine, 20)
        forms = [Gallery(case.d_g, cosine=cosine), Gallery(case.d_g, cosine=cosine, chunk_rows=1000),
                 Gallery([case.d_g[:1000], case.g[1000:2000], torch.from_numpy(case.g[2000:])], cosine=cosine),
                 Gallery([case.d_g[:5], case.d_g[5:]], cosine=cosine)]            # a chunk of fewer rows than k
        for gal in forms:
            idx, val = gal.search(case.d_q, k=20)
            assert idx.dtype == torch.int32 and val.dtype == torch.float32 and idx.shape == val.shape == (67, 20)
            assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(bits(val.cpu().numpy()), rv), (cosine, len(gal.chunks))
            if cosine:
                assert np.array_equal(bits(gal.inv_norm.cpu().numpy()), bits(case.w))
        with pytest.raises(ValueError):
            forms[0].search(case.d_q, k=65)


# ---------------------------------------------------------------- refusals
def test_search_refusals(H):
    """each refused before anything is launched: idx, val, the workspace and their guards keep their fill"""
    case = random_case(5, 1000, 64)
    nq, rows, dim, k = 5, 1000, 64, 16
    nws = workspace_bytes(H, nq, rows, dim, k, 4)
    whole, pay = guarded(nws + 2 * 4 * nq * 64 + 64)
    ws, idx, val = pay[:nws], pay[nws:nws + 4 * nq * 64], pay[nws + 4 * nq * 64:nws + 8 * nq * 64]
    fn = H.lib.ivit_search_topk
    q, g, w = case.d_q, case.d_g, case.d_w

    def call(query=P(q), nq_=nq, gallery=P(g), rows_=rows, dim_=dim, weight=P(w), k_=k, base=0, splits=4, ws_=P(ws), bytes_=nws, idx_=P(idx), val_=P(val)):
        return fn(H.h, query, nq_, gallery, rows_, dim_, weight, k_, base, splits, ws_, bytes_, idx_, val_)

    INV, UNS = _lib.IVIT_ERR_INVALID, _lib.IVIT_ERR_UNSUPPORTED
    assert call(k_=0) == INV and call(k_=65) == INV
    assert call(rows_=10, k_=11) == INV                           # k > rows
    assert call(dim_=96) == UNS and call(dim_=0) == UNS and call(dim_=1088) == UNS
    assert call(bytes_=nws - 1) == INV and b"workspace" in H.lib.ivit_last_error(H.h)
    assert call(query=_P(q.data_ptr() + 4)) == INV and b"query" in H.lib.ivit_last_error(H.h)
    assert call(gallery=_P(g.data_ptr() + 8), rows_=rows - 1) == INV and b"gallery" in H.lib.ivit_last_error(H.h)
    assert call(ws_=_P(ws.data_ptr() + 4), bytes_=nws) == INV
    assert call(val_=_P(idx.data_ptr() + 4 * nq * k - 4)) == INV and b"overlap" in H.lib.ivit_last_error(H.h)       # idx over val
    err = H.lib.ivit_last_error(H.h)
    assert b"idx" in err and b"val" in err
    assert call(idx_=_P(ws.data_ptr() + nws - 4)) == INV and b"overlap" in H.lib.ivit_last_error(H.h)               # idx over the workspace
    err = H.lib.ivit_last_error(H.h)
    assert b"idx" in err and b"workspace" in err
    assert call(val_=P(ws)) == INV and b"overlap" in H.lib.ivit_last_error(H.h)
    assert call(idx_=_P(g.data_ptr() + 64)) == INV and call(idx_=P(q)) == INV and call(val_=P(w)) == INV           # outputs over inputs
    assert call(base=TOP - rows + 1) == INV and call(base=TOP) == INV and call(base=-1) == INV
    assert call(splits=-1) == INV and call(splits=65536) == INV and call(nq_=-1) == INV
    assert call(query=None) == INV and call(gallery=None) == INV and call(idx_=None) == INV and call(ws_=None) == INV
    assert call(nq_=0) == _lib.IVIT_OK                            # nothing to do: nothing launched
    n = ctypes.c_size_t(77)
    wb = H.lib.ivit_search_workspace_bytes
    assert wb(H.h, nq, rows, 96, k, 0, ctypes.byref(n)) == UNS and wb(H.h, nq, rows, dim, 65, 0, ctypes.byref(n)) == INV
    assert wb(H.h, nq, rows, dim, k, 0, None) == INV and n.value == 77
    mg = H.lib.ivit_search_merge
    ci, cv = dev(np.zeros((nq, 32), np.int32)), dev(np.zeros((nq, 32), np.float32))
    assert mg(H.h, P(ci), P(cv), nq, 32, 0, P(idx), P(val)) == INV and mg(H.h, P(ci), P(cv), nq, 32, 65, P(idx), P(val)) == INV
    assert mg(H.h, P(ci), P(cv), nq, 32, 33, P(idx), P(val)) == INV                                                  # ncand < k
    assert mg(H.h, P(ci), P(cv), nq, 32, 16, P(idx), P(idx)) == INV and mg(H.h, P(ci), P(cv), nq, 32, 16, P(ci), P(val)) == INV
    assert mg(H.h, None, P(cv), nq, 32, 16, P(idx), P(val)) == INV
    torch.cuda.synchronize()
    assert np.all(whole.cpu().numpy() == FILL), "a refused call wrote"
    assert call() == _lib.IVIT_OK                                 # and the same arguments, unharmed, are accepted
    torch.cuda.synchronize()
    ri, rv = case.reference(True, k)
    assert np.array_equal(idx.cpu().numpy().view(np.int32)[:nq * k].reshape(nq, k), ri)
    assert np.array_equal(val.cpu().numpy().view(np.uint32)[:nq * k].reshape(nq, k), rv)
    assert guards_intact(whole, pay.numel())


# ---------------------------------------------------------------- end to end on the engines
def _engine(fname):
    g = load_golden(fname)
    if str(g["cfg_name"]) in iv.SWIN_CONFIGS:
        from ivit_amd.swin_engine import SwinEngine
        cfg = iv.SWIN_CONFIGS[str(g["cfg_name"])]
        eng = SwinEngine(cfg, iv.make_swin_weights(cfg, int(g["seed"])), golden_scales(g))
    else:
        from ivit_amd.engine import ViTEngine
        cfg = iv.CONFIGS[str(g["cfg_name"])]
        eng = ViTEngine.from_float(cfg, iv.make_vit_weights(cfg, int(g["seed"])), golden_scales(g))
    return cfg, eng


@pytest.mark.parametrize("fname", ["micro_vit2h_b3.npz", "micro_swin_b2.npz", "deit_tiny_b1.npz"])
def test_retrieve_and_knn_evaluate_end_to_end(fname):
    cfg, eng = _engine(fname)
    n_gal, n_cls, k = 12, 3, 5
    gal_images = torch.from_numpy(iv.make_images_int8(cfg, n_gal, seed=31)).cuda()
    labels = np.arange(n_gal) % n_cls
    fresh = torch.from_numpy(iv.make_images_int8(cfg, 3, seed=32)).cuda()
    queries = torch.cat([fresh, gal_images[7:8], gal_images[2:3]]).contiguous()          # two queries ARE gallery images
    qlabels = np.array([0, 1, 2, 7 % n_cls, 2 % n_cls])
    before = eng.forward(queries, copy=True)

    feat8, scale = embed8(eng, [gal_images[:5], (gal_images[5:9], None), gal_images[9:]])
    assert feat8.dtype == torch.int8 and feat8.shape == (n_gal, eng.num_features) and scale == float(eng.feature_scale_host())
    assert torch.equal(feat8[:5], eng.features(gal_images[:5])[0])
    g8 = feat8.cpu().numpy()
    for cosine in (True, False):
        gallery = Gallery(feat8, labels=labels, cosine=cosine)
        assert gallery.num_classes == n_cls and gallery.rows == n_gal
        idx, val, q8 = eng.retrieve(queries, gallery, k=k, copy=True)
        assert torch.equal(q8, eng.features(queries)[0])
        ri, rv = search_reference(q8.cpu().numpy(), g8, inv_norms_reference(g8) if cosine else None, k)
        assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(bits(val.cpu().numpy()), bits(rv)), cosine
        idx2 = eng.retrieve(queries, gallery, k=k, nslices=2)[0]
        assert torch.equal(idx2, idx)
        if cosine:                                                # a query that IS a gallery image comes back first
            assert idx[3, 0].item() == 7 and idx[4, 0].item() == 2
            assert torch.equal(q8[3], feat8[7]) and torch.equal(q8[4], feat8[2])
        qn = query_inv_norms(q8) if cosine else None
        order, vote = knn_classify(idx, val, gallery.labels, n_cls, T=0.07 if cosine else 1.0e6, query_inv_norm=qn)
        worder, wvote = knn_reference(ri, rv, labels, n_cls, T=0.07 if cosine else 1.0e6, query_inv_norm=None if qn is None else qn.cpu().numpy())
        assert np.array_equal(order.cpu().numpy(), worder)
        assert np.allclose(vote.cpu().numpy(), wvote, rtol=1e-12, atol=0)       # torch's and numpy's float64 exp may differ in the last bit
        res = knn_evaluate(eng, gallery, [(queries[:3], qlabels[:3]), (queries[3:], qlabels[3:])], k=k, T=0.07 if cosine else 1.0e6, topk=(1, 2))
        hits = {j: int(sum(int(ql in worder[b, :j]) for b, ql in enumerate(qlabels))) for j in (1, 2)}
        assert res == {"n": 5, "correct": hits, "acc": {j: 100.0 * hits[j] / 5 for j in (1, 2)}}
    after = eng.forward(queries)
    assert torch.equal(before, after)


# ---------------------------------------------------------------- hipGraph
def test_search_topk_captured_in_a_graph_replays_on_new_queries(H):
    case, other = random_case(67, 4099, 192), random_case(67, 1000, 192)
    k, nq, rows, dim = 17, 67, 4099, 192
    stream = torch.cuda.Stream()
    h2 = _lib.Handle(0, stream.cuda_stream)
    nws = workspace_bytes(h2, nq, rows, dim, k, 0)
    qbuf = case.d_q.clone()
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(nq, k, dtype=torch.int32, device="cuda")
    val = torch.zeros(nq, k, dtype=torch.float32, device="cuda")
    args = (P(qbuf), nq, P(case.d_g), rows, dim, P(case.d_w), k, 0, 0, P(ws), nws, P(idx), P(val))
    torch.cuda.synchronize()
    # eager once, against the reference (a kernel's first launch may be captured as well: tests/test_stream_graph_contract_gpu.py)
    with torch.cuda.stream(stream):
        h2.call("ivit_search_topk", *args)
    stream.synchronize()
    ri, rv = case.reference(True, k)
    assert np.array_equal(idx.cpu().numpy(), ri)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
        h2.call("ivit_search_topk", *args)
    idx.zero_()
    val.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(bits(val.cpu().numpy()), rv)
    qbuf.copy_(other.d_q)                                         # a second batch in the same buffer
    graph.replay()
    torch.cuda.synchronize()
    wi, wv = search_reference(other.q, case.g, case.w, k)
    assert np.array_equal(idx.cpu().numpy(), wi) and np.array_equal(bits(val.cpu().numpy()), bits(wv))
    assert not np.array_equal(wi, ri)
