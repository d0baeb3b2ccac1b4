"""HDBSCAN on the device (include/ivit_hdbscan.h): exact equality of integers and float bits against the numpy statements
(`predict.hdbscan_reference`, `predict.hdbscan_labels_reference`), no tolerance anywhere.  The core similarities at every width, row
count, both candidate-list sizes and the inputs that tie or compact most; the mutual-reachability forest on the same grid; one tree
against every DBSCAN*; the entries by hand between guards, refusals, a hipGraph of a whole run; the engines end to end."""
import ctypes
import math
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib, cluster  # noqa: E402
from ivit_amd.predict import (embed8, hdbscan_fit, hdbscan_labels_reference, hdbscan_reference, inv_norms_reference,  # noqa: E402
                              mutual_reachability_reference)
from test_density_gpu import CHAIN_THR, blobs, chains  # noqa: E402
from test_range_gpu import LOW, Guarded, H, _engine, dev  # noqa: E402,F401

_P = ctypes.c_void_p
ROWS = (1, 2, 31, 33, 97, 129, 300)                       # no pair, one pair, tile, wavefront, workgroup, several parts
SPLITS = (0, 1, 2, 3, 7)


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, np.float32).view(np.uint32)


def same(tree, want):
    got = [t.cpu().numpy() for t in (tree.u, tree.v, tree.val)]
    return all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want)) and np.array_equal(bits(got[2]), bits(want[2]))


@pytest.mark.parametrize("cosine", [False, True])
@pytest.mark.parametrize("dim", [64, 192, 1024])          # KS = 1, 3 (prefetch), 16 (no prefetch)
def test_core_similarity(dim, cosine):
    case = 0
    for rows in ROWS:
        x = blobs(rows, dim)
        w = inv_norms_reference(x) if cosine else None
        for min_pts in sorted({min(k, rows) for k in (1, 2, 16, 17, 64)}):                 # 64 slots up to 16, 128 above
            got = cluster.core_similarity(dev(x), min_pts, cosine=cosine, splits=SPLITS[case % 5])
            case += 1
            assert np.array_equal(bits(got), bits(mutual_reachability_reference(x, w, min_pts)[0])), (rows, min_pts)


@pytest.mark.parametrize("min_pts", [5, 16, 40])
def test_core_similarity_ties_and_ascending_scores(min_pts):
    same_rows = np.tile(blobs(1, 64), (300, 1))            # everything ties: the multiset rule decides
    rising = np.zeros((300, 64), np.int8)                  # row 0's scores ascend in g: every score survives, compaction every few tiles
    rising[:, 0], rising[:, 1] = 1, np.arange(300) % 100 + 1
    rising[:, 2] = np.arange(300) // 100
    rising[0, 1:3] = 1, 100
    assert (np.diff(rising[1:].astype(np.int32) @ rising[0].astype(np.int32)) > 0).all()
    for x in (same_rows, rising):
        for splits in (1, 3):
            got = cluster.core_similarity(dev(x), min_pts, cosine=False, splits=splits)
            assert np.array_equal(bits(got), bits(mutual_reachability_reference(x, None, min_pts)[0]))


def test_core_is_the_degree_threshold(H):
    x, min_pts = blobs(300, 192, seed=9), 5
    d, w = dev(x), dev(inv_norms_reference(x))
    core = cluster.core_similarity(d, min_pts)
    t = float(np.sort(core.cpu().numpy())[150])            # a value some pair attains: >= on the boundary
    n = ctypes.c_size_t()
    H.call("ivit_density_workspace_bytes", 300, 192, 0, ctypes.byref(n))
    ws, degree = torch.empty(n.value, dtype=torch.uint8, device="cuda"), torch.empty(300, dtype=torch.int32, device="cuda")
    H.call("ivit_density_degree", _P(d.data_ptr()), 300, 192, _P(w.data_ptr()), t, 0, _P(ws.data_ptr()), n.value, _P(degree.data_ptr()))
    is_core = (degree >= min_pts).cpu().numpy()
    assert np.array_equal(core.cpu().numpy() >= np.float32(t), is_core) and 0 < is_core.sum() < 300


@pytest.mark.parametrize("cosine", [False, True])
@pytest.mark.parametrize("dim", [64, 192, 1024])
def test_reach_forest(dim, cosine):
    case, forests = 0, 0
    for rows in ROWS:
        x = blobs(rows, dim)
        w = inv_norms_reference(x) if cosine else None
        for min_pts in sorted({min(k, rows) for k in (1, 5)}):
            m = np.sort(mutual_reachability_reference(x, w, min_pts)[1][np.triu_indices(rows, 1)])
            for floor in (None,) + ((m[(len(m) * 9) // 10],) if rows > 1 else ()):
                want = hdbscan_reference(x, w, min_pts, floor)
                _, core, tree, _ = cluster.hdbscan(dev(x), 5, min_pts, cosine=cosine, floor=floor, splits=SPLITS[case % 5])
                case += 1
                assert np.array_equal(bits(core), bits(want[0])) and same(tree, want[1:]) and tree.rounds <= math.ceil(math.log2(rows)), (rows, min_pts, floor)
                if min_pts == 1:
                    assert same(cluster.single_linkage(dev(x), cosine=cosine, floor=floor), want[1:])
                if floor is not None:
                    forests += 2 <= rows - len(want[1]) <= rows - 1
    assert forests >= 1                                    # of the reference: a floor that leaves a forest, neither a tree nor single rows


@pytest.mark.parametrize("floor", [CHAIN_THR, None])
@pytest.mark.parametrize("min_pts", [1, 2, 3])
def test_reach_forest_where_values_tie(floor, min_pts):
    for x in (chains(300, 31, seed=300)[0], chains(63, 63, seed=63)[0], np.tile(blobs(1, 64), (97, 1))):
        want = hdbscan_reference(x, None, min_pts, floor)
        _, core, tree, _ = cluster.hdbscan(dev(x), 5, min_pts, cosine=False, floor=floor, splits=3)
        assert np.array_equal(bits(core), bits(want[0])) and same(tree, want[1:])


def test_one_tree_every_dbscan_star():
    x, min_pts = blobs(300, 192, seed=9), 5
    x[4] = 0                                               # a row of zeros: its cosine with every row is 0
    d = dev(x)
    _, core, tree, _ = cluster.hdbscan(d, 5, min_pts)
    core = core.cpu().numpy()
    for t in (np.sort(core)[200], np.sort(core)[100]):     # thresholds attained exactly
        label, is_core = (a.cpu().numpy() for a in cluster.dbscan(d, float(t), min_pts)[:2])
        assert np.array_equal(is_core, core >= t) and 0 < is_core.sum() < 300
        group = tree.cut(t)                                # among core rows m >= t is v >= t; any other row has no edge at t
        assert np.array_equal(group[is_core], label[is_core]) and np.array_equal(group[~is_core], np.flatnonzero(~is_core))


def by_hand(H, x, w, min_pts, floor, splits, past=0):
    """the C entries stepped by hand until merged == 0 or one component, then `past` rounds more, which must change no byte -> core,
    the sorted edge set and the state; every output and both workspaces between guards"""
    rows, dim = x.shape
    n, nc = ctypes.c_size_t(), ctypes.c_size_t()
    H.call("ivit_linkage_workspace_bytes", rows, dim, splits, ctypes.byref(n))
    H.call("ivit_core_workspace_bytes", rows, dim, min_pts, splits, ctypes.byref(nc))
    d_x, d_w = dev(x), dev(w)
    ws, cws, core = Guarded(n.value), Guarded(nc.value), Guarded(4 * rows)
    run = [Guarded(4 * rows), Guarded(rows), Guarded(4 * rows), Guarded(4 * rows), Guarded(4 * rows), Guarded(16)]
    scan = (_P(d_x.data_ptr()), rows, dim, _P(d_w.data_ptr()))
    H.call("ivit_core_similarity", *scan, min_pts, splits, cws.ptr, nc.value, core.ptr)
    H.call("ivit_linkage_init", rows, *(g.ptr for g in run))
    state = lambda: run[5].payload().view(np.int32).copy()      # noqa: E731
    args = scan + (core.ptr, float(floor), splits, ws.ptr, n.value) + tuple(g.ptr for g in run)
    while state()[1] != 0:
        H.call("ivit_reach_round", *args)
        assert state()[2] <= math.ceil(math.log2(rows))
    before = [g.payload().copy() for g in run + [core]]
    for _ in range(past):
        H.call("ivit_reach_round", *args)
    torch.cuda.synchronize()
    assert all(np.array_equal(g.payload(), b) for g, b in zip(run + [core], before)), "a round past the end wrote"
    assert all(g.guards_intact() for g in [ws, cws, core] + run), "wrote outside an output"
    assert np.array_equal(d_x.cpu().numpy(), x) and np.array_equal(d_w.cpu().numpy(), w), "an input was written"
    u, v, val = run[2].payload().view(np.int32), run[3].payload().view(np.int32), run[4].payload().view(np.float32)
    order = np.lexsort((v[u >= 0], u[u >= 0], -val[u >= 0]))
    return [core.payload().view(np.float32).copy()] + [a[u >= 0][order] for a in (u, v, val)], state()


def test_hdbscan_entries_by_hand(H):
    x = blobs(300, 192, seed=2)
    w = inv_norms_reference(x)
    for floor in (-np.inf, 0.8):
        want = hdbscan_reference(x, w, 5, floor)
        got, state = by_hand(H, x, w, 5, floor, splits=3, past=3)
        assert all(a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, want))
        assert state[0] == 300 - len(want[1]) and state[1] == 0
        for splits in (1, 2, 7):
            assert all(np.array_equal(a, b) for a, b in zip(by_hand(H, x, w, 5, floor, splits)[0], got)), splits


def test_hdbscan_refusals(H):
    """each refused before anything is launched: every output and the workspace keep their fill"""
    x, rows, dim = dev(blobs(97, 64)), 97, 64
    n, nc = ctypes.c_size_t(), ctypes.c_size_t()
    H.call("ivit_linkage_workspace_bytes", rows, dim, 2, ctypes.byref(n))
    H.call("ivit_core_workspace_bytes", rows, dim, 64, 2, ctypes.byref(nc))
    size = max(n.value, nc.value)
    arena = Guarded(size + 6 * 4 * rows + 16)
    ws = arena.ptr.value
    comp, u, v, val, done, core = (ws + size + 4 * rows * i for i in range(6))
    state = core + 4 * rows
    good = torch.zeros(rows, dtype=torch.float32, device="cuda")
    INV, UNS, lib = _lib.IVIT_ERR_INVALID, _lib.IVIT_ERR_UNSUPPORTED, H.lib
    err = lambda: lib.ivit_last_error(H.h)                  # noqa: E731

    def call(x_=x.data_ptr(), rows_=rows, dim_=dim, core_=good.data_ptr(), floor=0.5, splits=2, ws_=ws, bytes_=size, comp_=comp, state_=state):
        return lib.ivit_reach_round(H.h, _P(x_), rows_, dim_, None, _P(core_), floor, splits, _P(ws_), bytes_, _P(comp_), _P(done), _P(u), _P(v), _P(val), _P(state_))

    def similarity(x_=x.data_ptr(), rows_=rows, dim_=dim, min_pts=5, ws_=ws, bytes_=size, core_=core):
        return lib.ivit_core_similarity(H.h, _P(x_), rows_, dim_, None, min_pts, 2, _P(ws_), bytes_, _P(core_))

    assert call(dim_=96) == UNS and call(rows_=0) == INV and call(splits=65536) == INV
    assert call(state_=None) == INV and b"null" in err() and call(x_=None) == INV and call(core_=None) == INV and b"null" in err()
    assert call(floor=float(np.nan)) == INV and b"floor" in err()
    assert call(bytes_=n.value - 1) == INV and b"workspace" in err()
    assert call(x_=x.data_ptr() + 4) == INV and b"x must be" in err() and call(comp_=comp + 2) == INV and b"comp must be" in err()
    assert call(core_=good.data_ptr() + 2) == INV and b"core must be" in err()
    assert call(core_=comp) == INV and b"overlap" in err() and b"core" in err() and b"comp" in err()
    assert call(comp_=x.data_ptr()) == INV and b"overlap" in err() and call(ws_=x.data_ptr()) == INV and b"overlap" in err()
    for bad in (0, 65, rows + 1):
        assert similarity(min_pts=bad) == INV and b"min_pts" in err(), bad
        assert lib.ivit_core_workspace_bytes(H.h, rows, dim, bad, 0, ctypes.byref(nc)) == INV
    assert similarity(rows_=20, min_pts=21) == INV and similarity(dim_=96) == UNS and similarity(core_=None) == INV and b"null" in err()
    assert similarity(core_=core + 2) == INV and b"core must be" in err() and similarity(bytes_=16) == INV and b"workspace" in err()
    assert similarity(core_=x.data_ptr()) == INV and b"overlap" in err() and similarity(core_=ws) == INV and b"overlap" in err()
    torch.cuda.synchronize()
    assert arena.untouched(), "a refused call wrote"
    assert similarity(min_pts=64) == 0 and lib.ivit_linkage_init(H.h, rows, _P(comp), _P(done), _P(u), _P(v), _P(val), _P(state)) == 0
    assert call(core_=core, floor=float(-np.inf)) == 0     # and the same arguments, unharmed, are accepted
    torch.cuda.synchronize()
    assert arena.guards_intact() and not arena.untouched()


def test_hdbscan_run_captured_in_a_graph():
    """the core pass, init and ceil(log2 rows) + 1 rounds in ONE graph: capture runs nothing; every replay leaves the eager bytes, on the
    captured rows and on new ones"""
    rows, dim, min_pts = 300, 64, 5
    stream = torch.cuda.Stream()
    h2 = _lib.Handle(0, stream.cuda_stream)
    n, nc = ctypes.c_size_t(), ctypes.c_size_t()
    h2.call("ivit_linkage_workspace_bytes", rows, dim, 0, ctypes.byref(n))
    h2.call("ivit_core_workspace_bytes", rows, dim, min_pts, 0, ctypes.byref(nc))
    d, ws, cws = dev(blobs(rows, dim)), torch.empty(n.value, dtype=torch.uint8, device="cuda"), torch.empty(nc.value, dtype=torch.uint8, device="cuda")
    comp, u, v, state = (torch.empty(m, dtype=torch.int32, device="cuda") for m in (rows, rows, rows, 4))
    done, val, core = torch.empty(rows, dtype=torch.uint8, device="cuda"), torch.empty(rows, dtype=torch.float32, device="cuda"), torch.empty(rows, dtype=torch.float32, device="cuda")
    run = tuple(_P(t.data_ptr()) for t in (comp, done, u, v, val, state))
    outs = (comp, done, u, v, val, state, core)

    def whole():
        h2.call("ivit_core_similarity", _P(d.data_ptr()), rows, dim, None, min_pts, 0, _P(cws.data_ptr()), nc.value, _P(core.data_ptr()))
        h2.call("ivit_linkage_init", rows, *run)
        for _ in range(math.ceil(math.log2(rows)) + 1):
            h2.call("ivit_reach_round", _P(d.data_ptr()), rows, dim, None, _P(core.data_ptr()), float(-np.inf), 0, _P(ws.data_ptr()), n.value, *run)

    with torch.cuda.stream(stream):
        whole()
    stream.synchronize()
    for t in (comp, u, v, state, core):
        t.fill_(-7)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
        whole()
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in (comp, u, v, state, core)), "the capture ran a launch"
    for x in (blobs(rows, dim), blobs(rows, dim, seed=5), chains(rows, 31, seed=2)[0]):
        d.copy_(dev(x))
        want = hdbscan_reference(x, None, min_pts)
        with torch.cuda.stream(stream):
            whole()
        stream.synchronize()
        eager = [t.cpu().numpy().copy() for t in outs]
        assert eager[5][0] == 1 and eager[5][1] == 0 and int((eager[2] < 0).sum()) == 1 and np.array_equal(bits(eager[6]), bits(want[0]))
        for _ in range(2):
            u.fill_(-7)
            core.fill_(-7)
            graph.replay()
            torch.cuda.synchronize()
            assert all(np.array_equal(t.cpu().numpy(), e) for t, e in zip(outs, eager))
        keep = eager[2] >= 0
        order = np.lexsort((eager[3][keep], eager[2][keep], -eager[4][keep]))
        assert all(np.array_equal(a[keep][order], b) for a, b in zip(eager[2:5], want[1:]))


@pytest.mark.parametrize("fname", ["micro_vit2h_b3.npz", "micro_swin_b2.npz"])
def test_hdbscan_fit_end_to_end(fname):
    cfg, eng = _engine(fname)
    images = torch.from_numpy(iv.make_images_int8(cfg, 12, seed=31)).cuda()
    batches = [images[:5], (torch.cat([images[5:], images[1:3], images[1:3]]).contiguous(), None)]       # images 1 and 2 three times each
    f8 = embed8(eng, batches)[0].cpu().numpy()
    label, core, tree, condensed, feat8 = hdbscan_fit(eng, batches, min_cluster_size=3, min_pts=2)
    w = inv_norms_reference(f8)
    want = hdbscan_reference(f8, w, 2)
    assert np.array_equal(feat8.cpu().numpy(), f8) and np.array_equal(bits(core), bits(want[0])) and same(tree, want[1:])
    assert np.array_equal(label.cpu().numpy(), hdbscan_labels_reference(mutual_reachability_reference(f8, w, 2)[1], 3)[0])
