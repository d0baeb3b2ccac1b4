"""Range search on the device (include/ivit_range.h).  Everything is bit-exact against the numpy statement
(`predict.range_reference`): array_equal on row_ptr, on idx and on the BITS of val, no tolerance anywhere.

The sweep crosses widths (KS = 1, 3, 16: the next-tile prefetch on and off), query counts (one query, a partial second wavefront, a
second workgroup), gallery sizes around the 32-row tile, the number of parts (0 = the library's choice, forced counts whose
boundaries fall inside a tile) and the three weightings.  The inputs come from -2 .. 2, so that many values tie, and the thresholds
from the REFERENCE's own values for the case: below the minimum (everything hits: idx rows are arange, which pins the order across
both lane halves and all four groups), above the maximum (nothing), the median, the 99th percentile, and a value that occurs, taken
exactly (a tie at the threshold is a hit).  `sweep_case` and `non_vacuity` are numpy only: what they assert of the reference (hits
strictly between nothing and everything, a tie, a row with hits in both parts of two) was checked on the CPU when the seeds were
chosen.  Then the independence of `splits`, signed zeros, the triangle in one piece and in chunk pairs, `capacity`, the memory
contract, the refusals, a hipGraph replay, the Python layer and the engines end to end."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import golden_scales, load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from ivit_amd.predict import find_duplicates, inv_norms_reference, range_reference  # noqa: E402
from ivit_amd.search import Gallery, cross_matches, duplicate_groups, duplicates  # noqa: E402

_P = ctypes.c_void_p
GUARD_BYTES = 4096
FILL = 0x5A
TOP = 2 ** 31 - 1
LOW = float(np.finfo(np.float32).min)                     # a finite threshold below every value: all of v


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


def P(t):
    return None if t is None else _P(t.data_ptr())


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Guarded:
    """`nbytes` of payload between two 4 KiB guards, everything filled with 0x5A; the payload may be empty (its address is still one)"""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.whole = torch.full((GUARD_BYTES + self.n + GUARD_BYTES,), FILL, dtype=torch.uint8, device="cuda")
        self.ptr = _P(self.whole.data_ptr() + GUARD_BYTES)

    def payload(self):
        return self.whole.cpu().numpy()[GUARD_BYTES:GUARD_BYTES + self.n]

    def guards_intact(self):
        w = self.whole.cpu().numpy()
        return bool(np.all(w[:GUARD_BYTES] == FILL) and np.all(w[GUARD_BYTES + self.n:] == FILL))

    def untouched(self):
        return bool(np.all(self.whole.cpu().numpy() == FILL))


def workspace_bytes(H, nq, rows, dim, splits):
    n = ctypes.c_size_t()
    H.call("ivit_range_workspace_bytes", nq, rows, dim, splits, ctypes.byref(n))
    return n.value


def run_range(H, d_q, d_g, d_w, d_qw, thr, ib=0, qb=0, tri=0, splits=0, capacity=None, with_val=True, room=0):
    """ivit_range_count, the total read back, ivit_range_fill -> (row_ptr int64 [nq + 1], idx int32 [capacity + room], val bits uint32
    [capacity + room]); capacity defaults to the total, `room` elements behind it belong to the buffers but not to the capacity.
    The guards around the workspace, row_ptr, idx and val must stay what they were."""
    (nq, dim), rows = d_q.shape, d_g.shape[0]
    nws = workspace_bytes(H, nq, rows, dim, splits)
    ws, rp = Guarded(nws), Guarded(8 * (nq + 1))
    common = (P(d_q), nq, P(d_g), rows, dim, P(d_w), P(d_qw), float(thr), ib, qb, tri, splits, ws.ptr, nws)
    H.call("ivit_range_count", *common, rp.ptr)
    torch.cuda.synchronize()
    row_ptr = rp.payload().view(np.int64).copy()
    cap = int(row_ptr[nq]) if capacity is None else capacity
    idx, val = Guarded(4 * (cap + room)), Guarded(4 * (cap + room))
    H.call("ivit_range_fill", *common, cap, idx.ptr, val.ptr if with_val else None)
    torch.cuda.synchronize()
    assert ws.guards_intact() and rp.guards_intact() and idx.guards_intact() and val.guards_intact(), "wrote outside an output"
    assert np.array_equal(rp.payload().view(np.int64), row_ptr), "the fill pass wrote row_ptr"
    if not with_val:
        assert val.untouched()
    return row_ptr, idx.payload().view(np.int32).copy(), val.payload().view(np.uint32).copy()


def check(H, d, ref, thr, what, **kw):
    """one count + fill on the device arrays d = (q, g, w, qw) against the reference (row_ptr, idx, val)"""
    rp, idx, val = run_range(H, *d, thr, **kw)
    assert np.array_equal(rp, ref[0]), (what, "row_ptr", np.argwhere(rp != ref[0])[:4].tolist())
    assert np.array_equal(idx, ref[1]), (what, "idx", np.argwhere(idx != ref[1])[:4].tolist())
    assert np.array_equal(val, bits(ref[2])), (what, "val", np.argwhere(val != bits(ref[2]))[:4].tolist())


# ---------------------------------------------------------------- the sweep
DIMS = [64, 192, 1024]          # KS = 1, 3 (prefetch), 16 (no prefetch)
NQ = [1, 33, 129]               # one query; a second, partial wavefront; a second workgroup
ROWS = [1, 31, 33, 97, 300]
SPLITS = [0, 1, 2, 3, 7]        # 97 / 2, 97 / 3, 300 / 7 ...: part boundaries inside a tile
WEIGHTS = ["none", "gallery", "both"]


@functools.lru_cache(maxsize=None)
def sweep_case(dim, nq, rows, weights):
    """numpy only: (q, g, w, qw), the five thresholds by name, and the reference for each"""
    rng = np.random.default_rng(7919 * dim + 101 * nq + rows)
    q = rng.integers(-2, 3, size=(nq, dim)).astype(np.int8)
    g = rng.integers(-2, 3, size=(rows, dim)).astype(np.int8)
    w = inv_norms_reference(g) if weights != "none" else None
    qw = inv_norms_reference(q) if weights == "both" else None
    v = range_reference(q, g, w, qw, LOW)[2].reshape(nq, rows)           # every value of the case
    thresholds = {"below": np.nextafter(v.min(), np.float32(-np.inf)), "above": np.nextafter(v.max(), np.float32(np.inf)),
                  "median": np.float32(np.median(v)), "p99": np.float32(np.percentile(v, 99)), "tie": v.flat[(v.size * 2) // 3]}
    refs = {name: range_reference(q, g, w, qw, t) for name, t in thresholds.items()}
    return (q, g, w, qw), thresholds, refs, v


def non_vacuity(dim, weights):
    """asserted on the reference alone.  A case of ONE score (nq = rows = 1) has no threshold strictly between nothing and
    everything: it is the only one exempt from the first condition."""
    both_parts = False
    for nq in NQ:
        for rows in ROWS:
            (q, g, w, qw), thresholds, refs, v = sweep_case(dim, nq, rows, weights)
            assert refs["below"][0][-1] == nq * rows and refs["above"][0][-1] == 0
            assert np.array_equal(refs["below"][1], np.tile(np.arange(rows, dtype=np.int32), nq))       # idx rows are arange
            if nq * rows > 1:
                for name in ("median", "p99"):
                    assert 0 < refs[name][0][-1] < nq * rows, (dim, nq, rows, weights, name)
            assert (v == thresholds["tie"]).any() and refs["tie"][0][-1] >= int((v == thresholds["tie"]).sum())
            per = -(-rows // 2)
            rp, idx, _ = refs["median"]
            both_parts |= any((idx[rp[b]:rp[b + 1]] < per).any() and (idx[rp[b]:rp[b + 1]] >= per).any() for b in range(nq))
    assert both_parts, (dim, weights)


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("dim", DIMS)
def test_range_sweep(H, dim, weights):
    non_vacuity(dim, weights)
    for nq in NQ:
        for rows in ROWS:
            host, thresholds, refs, _ = sweep_case(dim, nq, rows, weights)
            d = tuple(dev(a) for a in host)
            for name, thr in thresholds.items():
                for splits in SPLITS:
                    check(H, d, refs[name], thr, (dim, nq, rows, weights, name, splits), splits=splits)


def test_range_result_does_not_depend_on_splits(H):
    """identical bytes for every number of parts, more parts than rows (empty parts) among them, at both ends of the index range"""
    host, thresholds, refs, _ = sweep_case(192, 129, 300, "both")
    d = tuple(dev(a) for a in host)
    for ib, qb in ((0, 0), (TOP - 300, TOP - 129)):
        outs = [run_range(H, *d, thresholds["median"], ib=ib, qb=qb, splits=s) for s in (0, 1, 2, 3, 7, 10, 299, 300, 400)]
        for o in outs[1:]:
            assert all(np.array_equal(a, b) for a, b in zip(o, outs[0]))
        assert np.array_equal(outs[0][0], refs["median"][0]) and np.array_equal(outs[0][1].astype(np.int64) - ib, refs["median"][1])
        assert np.array_equal(outs[0][2], bits(refs["median"][2]))


# ---------------------------------------------------------------- signed zeros
def test_range_signed_zeros(H):
    """dot products of 0 under weights of both signs: +0.0 and -0.0 are both hits at a threshold of +0.0 and of -0.0, val keeps the sign"""
    rng = np.random.default_rng(12)
    q = rng.integers(-2, 3, size=(33, 64)).astype(np.int8)
    g = rng.integers(-2, 3, size=(97, 64)).astype(np.int8)
    g[::3] = 0                                                # dot 0 against every query
    q[5] = 0
    w = np.where(np.arange(97) % 2 == 0, np.float32(0.25), np.float32(-0.25)).astype(np.float32)
    w[10:14] = [0.0, -0.0, 0.0, -0.0]
    qw = np.where(np.arange(33) % 5 == 0, np.float32(-1.5), np.float32(1.5)).astype(np.float32)
    for weights in ((w, None), (w, qw)):
        d = (dev(q), dev(g), dev(weights[0]), dev(weights[1]))
        ref_p, ref_n = range_reference(q, g, *weights, 0.0), range_reference(q, g, *weights, -0.0)
        assert (bits(ref_p[2]) == 0x80000000).any() and (bits(ref_p[2]) == 0).any() and (ref_p[2] > 0).any()
        assert all(np.array_equal(a, b) for a, b in zip(ref_p[:2], ref_n[:2])) and np.array_equal(bits(ref_p[2]), bits(ref_n[2]))
        v = range_reference(q, g, *weights, LOW)[2]
        assert ref_p[0][-1] == int((v >= 0).sum()) and int((v == 0).sum()) > 33 * 30      # every zero of either sign is among the hits
        for thr in (0.0, -0.0):
            for splits in (0, 2, 7):
                check(H, d, ref_p, thr, ("signed zeros", thr, splits), splits=splits)


# ---------------------------------------------------------------- the triangle
def test_range_triangle_one_piece_and_chunk_pairs(H):
    """nq = rows = 97, the set against itself: every pair i < j once; the same pairs from chunk pairs whose tiles lie across, wholly above
    and wholly below the diagonal"""
    rng = np.random.default_rng(21)
    x = rng.integers(-2, 3, size=(97, 192)).astype(np.int8)
    x[40], x[96], x[33] = x[3], x[3], x[31]                   # planted duplicates, across tile and wavefront boundaries
    w = inv_norms_reference(x)
    d_x, d_w = dev(x), dev(w)
    v = range_reference(x, x, w, w, LOW)[2]
    for thr in (np.float32(np.median(v)), np.float32(0.999), LOW):
        for base in (0, 1000, TOP - 97):
            ref = range_reference(x, x, w, w, thr, base, base, True)
            assert ref[0][-1] > 0 and (ref[1].astype(np.int64) - base > np.repeat(np.arange(97), np.diff(ref[0]))).all()
            for splits in (0, 2, 3):
                check(H, (d_x, d_x, d_w, d_w), ref, thr, ("triangle", float(thr), base, splits), ib=base, qb=base, tri=1, splits=splits)
        whole = range_reference(x, x, w, w, thr, 0, 0, True)
        want = {(b, int(j)): int(u) for b in range(97) for j, u in zip(whole[1][whole[0][b]:whole[0][b + 1]], bits(whole[2][whole[0][b]:whole[0][b + 1]]))}
        cuts = [0, 32, 64, 97]                                # query_base 64 / index_base 32: wholly below; 32 / 64: wholly above
        got = {}
        for a0, a1 in zip(cuts[:-1], cuts[1:]):
            for b0, b1 in zip(cuts[:-1], cuts[1:]):
                ref = range_reference(x[a0:a1], x[b0:b1], w[b0:b1], w[a0:a1], thr, b0, a0, True)
                rp, idx, val = run_range(H, d_x[a0:a1], d_x[b0:b1], d_w[b0:b1], d_w[a0:a1], thr, ib=b0, qb=a0, tri=1)
                assert np.array_equal(rp, ref[0]) and np.array_equal(idx, ref[1]) and np.array_equal(val, bits(ref[2])), (a0, b0)
                if b0 < a0:
                    assert rp[-1] == 0
                if b0 > a0 and thr == LOW:
                    assert rp[-1] == (a1 - a0) * (b1 - b0)
                for b in range(a1 - a0):
                    got.update({(a0 + b, int(j)): int(u) for j, u in zip(idx[rp[b]:rp[b + 1]], val[rp[b]:rp[b + 1]])})
        assert got == want
    # a diagonal that no tile boundary knows of: odd bases, the queries ahead of and behind the gallery rows
    for ib, qb in ((5, 0), (0, 5), (17, 50), (50, 17), (0, 200), (200, 0)):
        ref = range_reference(x, x, w, w, LOW, ib, qb, True)
        for splits in (0, 2):
            check(H, (d_x, d_x, d_w, d_w), ref, LOW, ("triangle, shifted", ib, qb, splits), ib=ib, qb=qb, tri=1, splits=splits)


# ---------------------------------------------------------------- capacity, the memory contract
def test_range_capacity_limits_what_is_written(H):
    host, thresholds, refs, _ = sweep_case(192, 129, 300, "both")
    d = tuple(dev(a) for a in host)
    ref = refs["p99"]
    total = int(ref[0][-1])
    assert total > 8
    for splits in (0, 7):
        for cap in (0, total - 3, total, total + 5):
            rp, idx, val = run_range(H, *d, thresholds["p99"], splits=splits, capacity=cap, room=16)
            n = min(cap, total)
            assert np.array_equal(rp, ref[0]), cap            # row_ptr is the same whatever the capacity
            assert np.array_equal(idx[:n], ref[1][:n]) and np.array_equal(val[:n], bits(ref[2])[:n]), cap
            assert np.all(idx[n:].view(np.uint8) == FILL) and np.all(val[n:].view(np.uint8) == FILL), cap


def test_range_memory_contract(H):
    """inputs byte-identical after the calls (each inside guards of its own), val == NULL accepted and not written"""
    host, thresholds, refs, _ = sweep_case(64, 33, 97, "both")
    arenas = []
    for a in host:
        g = Guarded(a.nbytes)
        g.whole[GUARD_BYTES:GUARD_BYTES + a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()
        arenas.append(g)
    before = [g.whole.cpu().numpy().copy() for g in arenas]

    class View:                                               # what run_range needs of a device tensor
        def __init__(self, arena, shape):
            self.arena, self.shape = arena, shape

        def data_ptr(self):
            return self.arena.ptr.value

    d = (View(arenas[0], host[0].shape), View(arenas[1], host[1].shape), View(arenas[2], host[2].shape), View(arenas[3], host[3].shape))
    for with_val in (True, False):
        rp, idx, val = run_range(H, *d, thresholds["median"], splits=3, with_val=with_val)
        assert np.array_equal(rp, refs["median"][0]) and np.array_equal(idx, refs["median"][1])
        if with_val:
            assert np.array_equal(val, bits(refs["median"][2]))
    for g, b in zip(arenas, before):
        assert np.array_equal(g.whole.cpu().numpy(), b), "an input was written"


# ---------------------------------------------------------------- refusals
def test_range_refusals(H):
    """each refused before anything is launched: the workspace, row_ptr, idx, val and their guards keep their fill"""
    host, thresholds, refs, _ = sweep_case(64, 33, 97, "both")
    q, g, w, qw = (dev(a) for a in host)
    nq, rows, dim, thr = 33, 97, 64, float(thresholds["median"])
    nws = workspace_bytes(H, nq, rows, dim, 4)
    cap = int(refs["median"][0][-1])
    arena = Guarded(nws + 8 * (nq + 1) + 8 * cap + 64)
    base = arena.ptr.value
    ws, rp, idx, val = base, base + nws, base + nws + 8 * (nq + 1), base + nws + 8 * (nq + 1) + 4 * cap
    INV, UNS, OK = _lib.IVIT_ERR_INVALID, _lib.IVIT_ERR_UNSUPPORTED, _lib.IVIT_OK
    err = lambda: H.lib.ivit_last_error(H.h)                  # noqa: E731

    def common(**kw):
        a = dict(query=q.data_ptr(), nq=nq, gallery=g.data_ptr(), rows=rows, dim=dim, weight=w.data_ptr(), qweight=qw.data_ptr(), thr=thr, ib=0, qb=0,
                 tri=0, splits=4, ws=ws, bytes=nws)
        a.update(kw)
        return (H.h, _P(a["query"]), a["nq"], _P(a["gallery"]), a["rows"], a["dim"], _P(a["weight"]), _P(a["qweight"]), a["thr"], a["ib"], a["qb"],
                a["tri"], a["splits"], _P(a["ws"]), a["bytes"])

    def count(row_ptr=rp, **kw):
        return H.lib.ivit_range_count(*common(**kw), _P(row_ptr))

    def fill(capacity=cap, idx_=idx, val_=val, **kw):
        return H.lib.ivit_range_fill(*common(**kw), capacity, _P(idx_), _P(val_))

    for call in (count, fill):
        assert call(query=None) == INV and call(gallery=None) == INV and call(ws=None) == INV
        assert call(dim=32) == UNS and call(dim=1088) == UNS and call(dim=96) == UNS
        assert call(query=q.data_ptr() + 4) == INV and b"query" in err()
        assert call(gallery=g.data_ptr() + 8, rows=rows - 1) == INV and b"gallery" in err()
        assert call(ws=ws + 4) == INV and b"workspace" in err()
        for bad in (np.inf, -np.inf, np.nan):
            assert call(thr=float(bad)) == INV and b"threshold" in err()
        assert call(bytes=nws - 1) == INV and b"workspace" in err()
        assert call(rows=0) == INV and call(rows=-1) == INV and call(nq=-1) == INV
        assert call(ib=TOP - rows + 1) == INV and call(ib=-1) == INV and call(qb=TOP - nq + 1) == INV and call(qb=-1) == INV
        assert call(splits=-1) == INV and call(splits=65536) == INV
        assert call(nq=0) == OK                               # nothing to do: nothing launched, nothing written
    assert count(row_ptr=None) == INV and fill(idx_=None) == INV
    assert count(row_ptr=rp + 4) == INV and b"row_ptr" in err()
    assert fill(capacity=-1) == INV and b"capacity" in err()
    assert fill(capacity=0) == OK
    # every overlap the header names: outputs over inputs, outputs over each other, "overlap" and both names in the message
    for name, ptr in (("query", q.data_ptr()), ("gallery", g.data_ptr() + 64), ("weight", w.data_ptr()), ("qweight", qw.data_ptr())):
        assert count(ws=ptr) == INV and b"overlap" in err() and name.encode() in err() and b"workspace" in err()
        assert count(row_ptr=ptr) == INV and b"overlap" in err() and name.encode() in err() and b"row_ptr" in err()
        assert fill(idx_=ptr) == INV and b"overlap" in err() and name.encode() in err() and b"idx" in err()
        assert fill(val_=ptr) == INV and b"overlap" in err() and name.encode() in err() and b"val" in err()
    assert count(row_ptr=ws + nws - 8) == INV and b"overlap" in err() and b"workspace" in err() and b"row_ptr" in err()
    assert fill(idx_=ws + 8) == INV and b"overlap" in err() and b"workspace" in err() and b"idx" in err()
    assert fill(val_=ws + nws - 4) == INV and b"overlap" in err() and b"workspace" in err() and b"val" in err()
    assert fill(val_=idx + 4 * cap - 4) == INV and b"overlap" in err() and b"idx" in err() and b"val" in err()
    n = ctypes.c_size_t(77)
    wb = H.lib.ivit_range_workspace_bytes
    assert wb(H.h, nq, rows, 32, 0, ctypes.byref(n)) == UNS and wb(H.h, nq, 0, dim, 0, ctypes.byref(n)) == INV
    assert wb(H.h, nq, rows, dim, 65536, ctypes.byref(n)) == INV and wb(H.h, TOP, rows, dim, 2, ctypes.byref(n)) == INV       # nq * parts
    assert wb(H.h, nq, rows, dim, 0, None) == INV and n.value == 77
    torch.cuda.synchronize()
    assert arena.untouched(), "a refused call wrote"
    assert count() == OK and fill() == OK                     # and the same arguments, unharmed, are accepted
    torch.cuda.synchronize()
    pay = arena.payload()
    assert np.array_equal(pay[nws:nws + 8 * (nq + 1)].view(np.int64), refs["median"][0])
    assert np.array_equal(pay[nws + 8 * (nq + 1):][:4 * cap].view(np.int32), refs["median"][1])
    assert np.array_equal(pay[nws + 8 * (nq + 1) + 4 * cap:][:4 * cap].view(np.uint32), bits(refs["median"][2]))
    assert arena.guards_intact()


# ---------------------------------------------------------------- hipGraph
def test_range_count_and_fill_captured_in_a_graph_replay_on_new_queries(H):
    host, thresholds, refs, _ = sweep_case(192, 129, 300, "gallery")
    other = np.random.default_rng(5).integers(-2, 3, size=(129, 192)).astype(np.int8)
    q, g, w, _ = host
    thr, nq, rows, dim = float(thresholds["p99"]), 129, 300, 192
    want = range_reference(other, g, w, None, thr)
    cap = max(int(refs["p99"][0][-1]), int(want[0][-1])) + 7                          # a fixed buffer, checked afterwards
    stream = torch.cuda.Stream()
    h2 = _lib.Handle(0, stream.cuda_stream)
    nws = workspace_bytes(h2, nq, rows, dim, 0)
    qbuf, d_g, d_w = dev(q), dev(g), dev(w)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    row_ptr = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    idx = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    val = torch.zeros(cap, dtype=torch.float32, device="cuda")
    common = (P(qbuf), nq, P(d_g), rows, dim, P(d_w), None, thr, 0, 0, 0, 0, P(ws), nws)

    def both():
        h2.call("ivit_range_count", *common, P(row_ptr))
        h2.call("ivit_range_fill", *common, cap, P(idx), P(val))

    def same(ref):
        n = int(ref[0][-1])
        return (np.array_equal(row_ptr.cpu().numpy(), ref[0]) and np.array_equal(idx.cpu().numpy()[:n], ref[1])
                and np.array_equal(bits(val.cpu().numpy())[:n], bits(ref[2])) and bool((idx.cpu().numpy()[n:] == -1).all()))

    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        both()                                                # eager once
    stream.synchronize()
    assert same(refs["p99"])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
        both()
    row_ptr.zero_()
    idx.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    assert same(refs["p99"])
    qbuf.copy_(dev(other))                                    # a second batch in the same buffer
    idx.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    assert same(want) and int(want[0][-1]) <= cap and not np.array_equal(want[0], refs["p99"][0])


# ---------------------------------------------------------------- the Python layer
def _csr_equal(got, ref):
    rp, idx, val = (t.cpu().numpy() for t in got)
    return (got[0].dtype == torch.int64 and got[1].dtype == torch.int32 and got[2].dtype == torch.float32 and np.array_equal(rp, ref[0])
            and np.array_equal(idx, ref[1]) and np.array_equal(bits(val), bits(ref[2])))


def test_gallery_within_does_not_depend_on_the_chunking(H):
    host, thresholds, _, _ = sweep_case(64, 33, 300, "both")
    q, g, w, qw = host
    d_q, d_g = dev(q), dev(g)
    for cosine in (True, False):
        forms = [Gallery(d_g, cosine=cosine), Gallery(d_g, cosine=cosine, chunk_rows=32), Gallery(d_g, cosine=cosine, chunk_rows=50),
                 Gallery([d_g[:100], g[100:170], torch.from_numpy(g[170:])], cosine=cosine)]          # host chunks among them
        v = range_reference(q, g, w if cosine else None, qw if cosine else None, LOW)[2]
        for thr in (np.float32(np.median(v)), np.float32(np.percentile(v, 99)), np.nextafter(v.max(), np.float32(np.inf))):
            ref = range_reference(q, g, w if cosine else None, qw if cosine else None, thr)
            tri = range_reference(q, g, w if cosine else None, qw if cosine else None, thr, 0, 40, True)
            for gal in forms:
                assert _csr_equal(gal.within(d_q, thr), ref), (cosine, len(gal.chunks), float(thr))
                assert _csr_equal(gal.within(d_q, thr, triangle=True, query_base=40), tri), (cosine, len(gal.chunks), float(thr))
        plain = range_reference(q, g, w if cosine else None, None, np.float32(1.0))                    # without the queries' weights
        assert _csr_equal(forms[1].within(d_q, 1.0, query_weight=None), plain)
        with pytest.raises(ValueError):
            forms[0].within(d_q, float("nan"))


def _pairs_reference(a, b, cosine, thr, triangle):
    wa, wb = (inv_norms_reference(a), inv_norms_reference(b)) if cosine else (None, None)
    rp, idx, val = range_reference(a, b, wb, wa, thr, 0, 0, triangle)
    return np.stack([np.repeat(np.arange(len(a)), np.diff(rp)), idx.astype(np.int64)], 1), val


def test_duplicates_and_cross_matches_equal_the_reference(H):
    rng = np.random.default_rng(33)
    x = rng.integers(-20, 21, size=(150, 64)).astype(np.int8)
    x[70], x[149], x[31] = x[4], x[4], x[32]                  # exact duplicates
    near = x[100].copy()
    near[:3] += 1
    x[12] = near                                              # a near duplicate
    y = rng.integers(-20, 21, size=(90, 64)).astype(np.int8)
    y[5], y[64], y[89] = x[4], x[100], x[149]                 # rows of x that leak into y
    for cosine, thr in ((True, 0.98), (False, float((x[100].astype(np.int32) ** 2).sum() - 500))):
        want_p, want_v = _pairs_reference(x, x, cosine, thr, True)
        assert {(4, 70), (4, 149), (70, 149), (31, 32), (12, 100)} <= set(map(tuple, want_p.tolist())) and len(want_p) < 40
        for form in (dev(x), [dev(x[:32]), x[32:80], dev(x[80:])]):
            for chunk_rows in (None, 50):
                pairs, val = duplicates(form, thr, cosine=cosine, chunk_rows=chunk_rows)
                assert pairs.dtype == torch.int64 and np.array_equal(pairs.cpu().numpy(), want_p) and np.array_equal(bits(val.cpu().numpy()), bits(want_v))
        group = duplicate_groups(pairs, 150)
        assert group[70] == group[149] == group[4] == 4 and group[32] == 31 and group[100] == 12 and (group == np.arange(150)).sum() == 150 - 4        # {4, 70, 149}, {31, 32}, {12, 100}: four rows go
        want_p, want_v = _pairs_reference(x, y, cosine, thr, False)
        assert {(4, 5), (70, 5), (149, 5), (100, 64), (4, 89)} <= set(map(tuple, want_p.tolist()))
        for chunk_rows in (None, 40):
            pairs, val = cross_matches(dev(x), dev(y), thr, cosine=cosine, chunk_rows=chunk_rows)
            assert np.array_equal(pairs.cpu().numpy(), want_p) and np.array_equal(bits(val.cpu().numpy()), bits(want_v))


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


@pytest.mark.parametrize("fname", ["micro_vit2h_b3.npz", "micro_swin_b2.npz"])
def test_retrieve_within_and_find_duplicates_end_to_end(fname):
    cfg, eng = _engine(fname)
    gal_images = torch.from_numpy(iv.make_images_int8(cfg, 12, seed=31)).cuda()
    fresh = torch.from_numpy(iv.make_images_int8(cfg, 3, seed=32)).cuda()
    queries = torch.cat([fresh, gal_images[7:8], gal_images[2:3]]).contiguous()          # two queries ARE gallery images
    before = eng.forward(queries, copy=True)
    g8_dev = eng.features(gal_images)[0].clone()
    g8 = g8_dev.cpu().numpy()
    for cosine in (True, False):
        gallery = Gallery(g8_dev, cosine=cosine)
        q8_ref = eng.features(queries)[0].cpu().numpy()
        w, qw = (inv_norms_reference(g8), inv_norms_reference(q8_ref)) if cosine else (None, None)
        v = range_reference(q8_ref, g8, w, qw, LOW)[2]
        for thr in (np.float32(np.median(v)), v.max()):
            row_ptr, idx, val, q8 = eng.retrieve_within(queries, gallery, thr)
            assert np.array_equal(q8.cpu().numpy(), q8_ref)
            ref = range_reference(q8_ref, g8, w, qw, thr)
            assert ref[0][-1] > 0 and _csr_equal((row_ptr, idx, val), ref), (cosine, float(thr))
        if cosine:                                            # a query that IS a gallery image finds it at a cosine of one
            row_ptr, idx, val, _ = eng.retrieve_within(queries, gallery, 0.9999)
            rp, ix = row_ptr.cpu().numpy(), idx.cpu().numpy()
            assert 7 in ix[rp[3]:rp[4]] and 2 in ix[rp[4]:rp[5]]
    batches = [gal_images[:5], (torch.cat([gal_images[5:8], gal_images[1:2]]).contiguous(), None), torch.cat([gal_images[8:], gal_images[6:7]]).contiguous()]
    pairs, val, feat8 = find_duplicates(eng, batches, 0.9999)                             # rows 8 and 13 repeat images 1 and 6
    f8 = feat8.cpu().numpy()
    assert f8.shape == (14, eng.num_features) and np.array_equal(f8[8], f8[1]) and np.array_equal(f8[13], f8[6])
    want_p, want_v = _pairs_reference(f8, f8, True, 0.9999, True)
    assert np.array_equal(pairs.cpu().numpy(), want_p) and np.array_equal(bits(val.cpu().numpy()), bits(want_v))
    assert {(1, 8), (6, 13)} <= set(map(tuple, want_p.tolist()))
    assert torch.equal(before, eng.forward(queries))
