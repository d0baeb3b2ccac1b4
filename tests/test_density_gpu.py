"""Density clustering on the device (include/ivit_density.h): exact equality of integers against the numpy statement
(`predict.dbscan_reference`), no tolerance anywhere.  Widths with the prefetch on and off, row counts around the tile, the wavefront and
the workgroup, both weightings, min_pts, parts; shuffled chains that need many sweeps; independence of `splits` and `check_every`;
the pair-list route on a threshold a pair attains exactly; the memory contract, refusals, a hipGraph replay; the engines end to end."""
import ctypes
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib, cluster  # noqa: E402
from ivit_amd.predict import dbscan_fit, dbscan_reference, embed8, inv_norms_reference, range_reference  # noqa: E402
from ivit_amd.search import duplicate_groups, duplicate_groups_device, duplicates  # noqa: E402
from test_range_gpu import LOW, Guarded, H, _engine, dev  # noqa: E402,F401

_P = ctypes.c_void_p
NONE = 2 ** 31 - 1


def blobs(rows, dim, seed=0):
    """a few centres plus noise, every seventh row on its own, a triple a - b - c per 40 rows: b = u, a = 0.6 u + p, c = 0.6 u + q on
    columns of their own: at a cosine of 0.8 and a dot product of 115 dim a and c reach b, not each other (border rows at min_pts 3)"""
    rng = np.random.default_rng(seed + 31 * dim + rows)
    x = rng.integers(-20, 21, size=(4, dim))[rng.integers(0, 4, size=rows)] + rng.integers(-3, 4, size=(rows, dim))
    x[::7] = rng.integers(-20, 21, size=x[::7].shape)
    for a, b, c in rng.permutation(rows)[:3 * (rows // 40)].reshape(-1, 3):
        u = np.where(np.arange(dim) < dim // 2, rng.choice([-5, 5], size=dim), 0)
        x[b], x[a], x[c] = 5 * u, 3 * u, 3 * u
        x[a, dim // 2:3 * dim // 4] = rng.choice([-13, 13], size=dim // 4)
        x[c, 3 * dim // 4:] = rng.choice([-13, 13], size=dim // 4)
    return x.astype(np.int8)


def chains(rows, length, seed):
    """dim 64.  Row c of a chain holds the same value in columns c and c + 1 of its block of columns: adjacent to the next row at a
    threshold of that value squared (CHAIN_THR) and not to the one after.  A chain per block of length + 1 columns and sign; the other
    rows are zeros; the row indices shuffled, so that the minimum has to travel"""
    x = np.zeros((rows, 64), np.int8)
    n = 0
    for block in range(64 // (length + 1)):
        for sign in (7, -7):
            if n + length <= rows:
                for c in range(length):
                    x[n + c, block * (length + 1) + c] = x[n + c, block * (length + 1) + c + 1] = sign
                n += length
    out = np.empty_like(x)
    out[np.random.default_rng(seed).permutation(rows)] = x
    return out, n // length


CHAIN_THR = 49.0


def by_hand(H, x, w, thr, min_pts, splits, past=0):
    """the C entries stepped by hand, `past` sweeps beyond the first that reports 0 -> degree, the converged label, out and the
    `changed` of every sweep.  Every output and the workspace lie between guards, which must stay what they were, as must the inputs"""
    rows, dim = x.shape
    n = ctypes.c_size_t()
    H.call("ivit_density_workspace_bytes", rows, dim, splits, ctypes.byref(n))
    words = ((rows + 31) // 32 + 63) // 64
    d_x, d_w = dev(x), dev(w)
    ws, degree, out, changed = Guarded(n.value), Guarded(4 * rows), Guarded(4 * rows), Guarded(4)
    label, dirty = [Guarded(4 * rows), Guarded(4 * rows)], [Guarded(8 * words), Guarded(8 * words)]
    get = lambda g, dt: g.payload().view(dt).copy()          # noqa: E731
    scan = (_P(d_x.data_ptr()), rows, dim, d_w is not None and _P(d_w.data_ptr()) or None, float(thr), splits, ws.ptr, n.value)
    H.call("ivit_density_degree", *scan, degree.ptr)
    H.call("ivit_density_init", degree.ptr, rows, min_pts, label[0].ptr, dirty[0].ptr)
    counts = []
    while past >= 0:
        a, b = len(counts) & 1, ~len(counts) & 1
        H.call("ivit_density_sweep", *scan, label[a].ptr, dirty[a].ptr, label[b].ptr, dirty[b].ptr, changed.ptr)
        counts.append(int(get(changed, np.int32)[0]))
        if counts[-1] == 0:
            assert np.array_equal(get(label[a], np.int32), get(label[b], np.int32)) and not get(dirty[b], np.uint64).any()
            past -= 1
        assert len(counts) <= rows + 8
    final = label[len(counts) & 1]
    H.call("ivit_density_border", *scan, final.ptr, out.ptr)
    torch.cuda.synchronize()
    assert all(g.guards_intact() for g in [ws, degree, out, changed] + label + dirty), "wrote outside an output"
    assert np.array_equal(d_x.cpu().numpy(), x) and (w is None or np.array_equal(d_w.cpu().numpy(), w)), "an input was written"
    return get(degree, np.int32), get(final, np.int32), get(out, np.int32), counts


@pytest.mark.parametrize("cosine", [False, True])
@pytest.mark.parametrize("dim", [64, 192, 1024])          # KS = 1, 3 (prefetch), 16 (no prefetch)
def test_dbscan_sweep(dim, cosine):
    case, clusters, noise, border = 0, 0, 0, 0
    for rows in (1, 31, 33, 97, 300):
        x = blobs(rows, dim)
        w = inv_norms_reference(x) if cosine else None
        thr = 0.8 if cosine else 115.0 * dim
        for min_pts in (1, 3, rows + 1):
            want = dbscan_reference(x, w, thr, min_pts)
            label, core, degree, sweeps = cluster.dbscan(dev(x), thr, min_pts, cosine=cosine, splits=(0, 1, 2, 3, 7)[case % 5])
            case += 1
            for got, ref, name in zip((label, core, degree), want, ("label", "core", "degree")):
                assert np.array_equal(got.cpu().numpy(), ref), (rows, min_pts, name)
            if min_pts == rows + 1:
                assert (want[0] == -1).all() and not want[1].any()
            elif rows == 300:
                clusters += len(np.unique(want[0][want[0] >= 0]))
                noise += int((want[0] < 0).sum())
                border += int(((want[0] >= 0) & ~want[1]).sum())
    assert clusters >= 6 and noise > 20 and border > 0     # of the reference: several clusters, noise rows and border rows


@pytest.mark.parametrize("rows,length", [(63, 63), (300, 31)])
@pytest.mark.parametrize("min_pts", [1, 3])
def test_dbscan_chains_need_many_sweeps(H, rows, length, min_pts):
    x, n = chains(rows, length, seed=rows)
    want = dbscan_reference(x, None, CHAIN_THR, min_pts)
    assert n == (1 if rows == 63 else 4) and len(np.unique(want[0][want[0] >= 0])) == n
    assert int(((want[0] >= 0) & ~want[1]).sum()) == (2 * n if min_pts == 3 else 0)          # at 3 the ends are border rows
    degree, final, out, counts = by_hand(H, x, None, CHAIN_THR, min_pts, splits=3)
    assert np.array_equal(out, want[0]) and np.array_equal(degree, want[2]) and np.array_equal(final != NONE, want[1])
    assert len(counts) >= 4 and counts[0] > 0 and (rows == 63 or min(counts[:-1]) < (rows + 31) // 32)   # several sweeps; later ones skip tiles


def test_dbscan_does_not_depend_on_splits_or_check_every(H):
    x, _ = chains(300, 31, seed=5)
    x[::9] = blobs(300, 64)[::9]
    want = dbscan_reference(x, None, CHAIN_THR, 3)
    d = dev(x)
    for splits in (1, 2, 3, 7):
        for check_every in (1, 4):
            label, core, degree, sweeps = cluster.dbscan(d, CHAIN_THR, 3, cosine=False, check_every=check_every, splits=splits)
            assert np.array_equal(label.cpu().numpy(), want[0]) and sweeps % check_every == 0, (splits, check_every)
    degree, final, out, counts = by_hand(H, x, None, CHAIN_THR, 3, splits=2, past=2)   # two sweeps past convergence: asserted inside
    assert counts[-3:] == [0, 0, 0] and counts[-4] > 0 and np.array_equal(out, want[0])


def test_duplicate_groups_device_is_duplicate_groups_of_duplicates():
    x = blobs(300, 192, seed=9)
    x[4] = 0                                               # a row of zeros: no neighbour, not even itself; its group is itself
    w = inv_norms_reference(x)
    v = np.sort(range_reference(x, x, w, w, LOW, 0, 0, True)[2])
    for thr in (v[(len(v) * 9) // 10], v[-200]):           # values some pair attains exactly: >= on the boundary
        d = dev(x)
        want = duplicate_groups(duplicates(d, thr)[0], 300)
        got = duplicate_groups_device(d, thr)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want) and 1 < len(np.unique(want)) < 300, float(thr)
        label = dbscan_reference(x, w, thr, 1)[0]
        assert label[4] == -1 and np.array_equal(np.where(label < 0, np.arange(300), label), want)


def test_dbscan_memory_contract(H):
    """guards around every output and the workspace, the inputs unchanged (asserted in by_hand), with weights and three parts"""
    x = blobs(300, 192, seed=2)
    w, want = inv_norms_reference(x), dbscan_reference(x, inv_norms_reference(x), 0.8, 3)
    degree, final, out, counts = by_hand(H, x, w, 0.8, 3, splits=3)
    assert np.array_equal(out, want[0]) and np.array_equal(degree, want[2]) and np.array_equal(final != NONE, want[1])


def test_dbscan_refusals(H):
    """each refused before anything is launched: every output and the workspace keep their fill"""
    x, rows, dim = dev(blobs(97, 64)), 97, 64
    n = ctypes.c_size_t()
    H.call("ivit_density_workspace_bytes", rows, dim, 2, ctypes.byref(n))
    arena = Guarded(n.value + 4 * 4 * rows + 2 * 8 + 16)
    ws = arena.ptr.value
    deg, lab_in, lab_out, out = (ws + n.value + 4 * rows * i for i in range(4))
    dirty_in, dirty_out, changed = (out + 4 * rows + 8 * i for i in range(3))
    INV, UNS, lib = _lib.IVIT_ERR_INVALID, _lib.IVIT_ERR_UNSUPPORTED, H.lib
    err = lambda: lib.ivit_last_error(H.h)                  # noqa: E731

    def calls(x_=x.data_ptr(), rows_=rows, dim_=dim, thr=0.5, splits=2, ws_=ws, bytes_=n.value, lab_out_=lab_out, only=slice(0, 3)):
        scan = (H.h, _P(x_), rows_, dim_, None, thr, splits, _P(ws_), bytes_)
        entries = (lambda: lib.ivit_density_degree(*scan, _P(deg)),
                   lambda: lib.ivit_density_sweep(*scan, _P(lab_in), _P(dirty_in), _P(lab_out_), _P(dirty_out), _P(changed)),
                   lambda: lib.ivit_density_border(*scan, _P(lab_in), _P(out)))
        return tuple(e() for e in entries[only])

    assert calls(dim_=96) == (UNS,) * 3 and calls(rows_=0) == (INV,) * 3 and calls(splits=65536) == (INV,) * 3
    for bad in (np.inf, np.nan):
        assert calls(thr=float(bad)) == (INV,) * 3 and b"threshold" in err()
    assert calls(bytes_=n.value - 1) == (INV,) * 3 and b"workspace" in err()
    assert calls(x_=x.data_ptr() + 4) == (INV,) * 3 and b"x must be" in err()
    assert calls(lab_out_=lab_in, only=slice(1, 2)) == (INV,) and b"overlap" in err() and b"label_in" in err() and b"label_out" in err()
    assert calls(ws_=x.data_ptr()) == (INV,) * 3 and b"overlap" in err()
    init = lambda rows_=rows, min_pts=2, lab=lab_in: lib.ivit_density_init(H.h, _P(deg), rows_, min_pts, _P(lab), _P(dirty_in))      # noqa: E731
    assert init(min_pts=0) == INV and b"min_pts" in err() and init(rows_=0) == INV and init(lab=deg) == INV and b"overlap" in err()
    assert lib.ivit_density_workspace_bytes(H.h, rows, 96, 0, ctypes.byref(n)) == UNS
    torch.cuda.synchronize()
    assert arena.untouched(), "a refused call wrote"
    assert calls(only=slice(0, 1)) == (0,) and init() == 0                 # and the same arguments, unharmed, are accepted
    torch.cuda.synchronize()
    assert arena.guards_intact() and not arena.untouched()


def test_dbscan_sweep_captured_in_a_graph(H):
    """a sweep captured on a side stream runs nothing before the launch; every replay leaves the bytes of the eager call"""
    x = chains(300, 31, seed=1)[0]
    stream = torch.cuda.Stream()
    h2 = _lib.Handle(0, stream.cuda_stream)
    n = ctypes.c_size_t()
    h2.call("ivit_density_workspace_bytes", 300, 64, 0, ctypes.byref(n))
    d, ws = dev(x), torch.empty(n.value, dtype=torch.uint8, device="cuda")
    degree, lab_in, lab_out = (torch.empty(300, dtype=torch.int32, device="cuda") for _ in range(3))
    dirty_in, dirty_out = (torch.empty(1, dtype=torch.int64, device="cuda") for _ in range(2))
    changed = torch.empty(1, dtype=torch.int32, device="cuda")
    scan = (_P(d.data_ptr()), 300, 64, None, CHAIN_THR, 0, _P(ws.data_ptr()), n.value)
    sweep = lambda: h2.call("ivit_density_sweep", *scan, *(_P(t.data_ptr()) for t in (lab_in, dirty_in, lab_out, dirty_out, changed)))      # noqa: E731
    outs = lambda: [t.cpu().numpy().copy() for t in (lab_out, dirty_out, changed)]      # noqa: E731
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        h2.call("ivit_density_degree", *scan, _P(degree.data_ptr()))
        h2.call("ivit_density_init", _P(degree.data_ptr()), 300, 1, _P(lab_in.data_ptr()), _P(dirty_in.data_ptr()))
        sweep()
    stream.synchronize()
    eager = outs()
    assert eager[2][0] > 0 and not np.array_equal(eager[0], lab_in.cpu().numpy())
    for t in (lab_out, dirty_out, changed):
        t.fill_(-7)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
        sweep()
    torch.cuda.synchronize()
    assert all((o == -7).all() for o in outs()), "the capture ran a launch"
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(a, b) for a, b in zip(outs(), eager))
        lab_out.fill_(-7)


@pytest.mark.parametrize("fname", ["micro_vit2h_b3.npz", "micro_swin_b2.npz"])
def test_dbscan_fit_end_to_end(fname):
    cfg, eng = _engine(fname)
    images = torch.from_numpy(iv.make_images_int8(cfg, 12, seed=31)).cuda()
    batches = [images[:5], (torch.cat([images[5:], images[1:3]]).contiguous(), None)]       # rows 12 and 13 repeat images 1 and 2
    f8 = embed8(eng, batches)[0].cpu().numpy()
    w = inv_norms_reference(f8)
    v = range_reference(f8, f8, w, w, LOW, 0, 0, True)[2]
    for thr, min_pts in ((np.float32(np.median(v)), 3), (np.float32(0.9999), 2)):
        label, core, degree, feat8 = dbscan_fit(eng, batches, thr, min_pts)
        want = dbscan_reference(f8, w, thr, min_pts)
        assert np.array_equal(feat8.cpu().numpy(), f8)
        assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip((label, core, degree), want))
    assert want[0][12] == want[0][1] == 1 and want[0][13] == want[0][2] == 2 and (want[0] >= 0).sum() >= 4
    compact, count = cluster.compact_labels(label)
    assert count == len(np.unique(want[0][want[0] >= 0])) and compact[1] == 0 and compact[13] == 1 and (compact[label < 0] == -1).all()
