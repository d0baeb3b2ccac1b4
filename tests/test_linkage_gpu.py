"""The single-linkage hierarchy on the device (include/ivit_linkage.h): exact equality of integers and float bits against the numpy
statement (`predict.linkage_reference`), no tolerance anywhere.  Widths with the prefetch on and off, row counts around the tile, the
wavefront and the workgroup, both weightings, parts, floors; shuffled chains and identical rows, where almost every value ties; the
cut against the existing device route; the memory contract, rounds past the end, refusals, a hipGraph of a whole run; the engines
end to end."""
import ctypes
import math
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib, cluster  # noqa: E402
from ivit_amd.predict import embed8, inv_norms_reference, linkage_fit, linkage_reference, range_reference  # noqa: E402
from ivit_amd.search import duplicate_groups_device  # noqa: E402
from test_density_gpu import CHAIN_THR, blobs, chains  # noqa: E402
from test_range_gpu import LOW, Guarded, H, _engine, dev  # noqa: E402,F401

_P = ctypes.c_void_p


def same(tree, want):
    """the Linkage's edges against the reference's, integers and float bits"""
    got = [t.cpu().numpy() for t in (tree.u, tree.v, tree.val)]
    return all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want)) and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))


@pytest.mark.parametrize("cosine", [False, True])
@pytest.mark.parametrize("dim", [64, 192, 1024])          # KS = 1, 3 (prefetch), 16 (no prefetch)
def test_single_linkage(dim, cosine):
    case, forests = 0, 0
    for rows in (1, 2, 31, 33, 97, 129, 300):             # no edge, one edge, tile, wavefront, workgroup, several parts
        x = blobs(rows, dim)
        w = inv_norms_reference(x) if cosine else None
        v = np.sort(range_reference(x, x, w, w, LOW, 0, 0, True)[2])                       # the values of the pairs i < j
        for floor in (None,) + ((v[(len(v) * 9) // 10],) if rows > 1 else ()):
            want = linkage_reference(x, w, floor)
            tree = cluster.single_linkage(dev(x), cosine=cosine, floor=floor, splits=(0, 1, 2, 3, 7)[case % 5])
            case += 1
            assert same(tree, want) and tree.rows == rows and tree.rounds <= math.ceil(math.log2(rows)), (rows, floor)
            if floor is not None:
                forests += 2 <= rows - len(want[0]) <= rows - 1
            elif rows == 300 and not cosine:
                assert len(want[0]) == 299 and len(np.unique(v)) < len(v) and tree.rounds >= 3                    # tied pairs; several rounds
    assert forests >= 1                                    # of the reference: a floor that leaves a forest, neither a tree nor single rows


@pytest.mark.parametrize("rows,length", [(63, 63), (300, 31)])
@pytest.mark.parametrize("floor", [CHAIN_THR, None])
def test_single_linkage_shuffled_chains(rows, length, floor):
    """almost all values tie and the hooks form long chains"""
    x, n = chains(rows, length, seed=rows)
    want = linkage_reference(x, None, floor)
    tree = cluster.single_linkage(dev(x), cosine=False, floor=floor, splits=3)
    assert same(tree, want) and len(want[0]) == (n * (length - 1) if floor else rows - 1) and 1 <= tree.rounds <= math.ceil(math.log2(rows))


def test_single_linkage_all_rows_identical():
    x = np.tile(blobs(1, 64), (97, 1))
    for cosine in (False, True):
        want = linkage_reference(x, inv_norms_reference(x) if cosine else None)
        assert same(cluster.single_linkage(dev(x), cosine=cosine), want) and len(np.unique(want[2])) == 1


def test_cut_is_duplicate_groups_device():
    x = blobs(300, 192, seed=9)
    x[4] = 0                                               # a row of zeros: its cosine with every row is 0
    w = inv_norms_reference(x)
    v = np.sort(range_reference(x, x, w, w, LOW, 0, 0, True)[2])
    d = dev(x)
    tree = cluster.single_linkage(d)
    for thr in (v[(len(v) * 9) // 10], v[-200]):           # values some pair attains exactly: >= on the boundary
        want = duplicate_groups_device(d, thr).cpu().numpy()
        assert np.array_equal(tree.cut(thr), want) and 1 < len(np.unique(want)) < 300, float(thr)
    assert np.array_equal(tree.cut_k(1), np.zeros(300, np.int64)) and len(np.unique(tree.cut_k(7))) == 7


def by_hand(H, x, w, floor, splits, past=0):
    """the C entries stepped by hand until merged == 0 or one component, then `past` rounds more, which must change no byte -> the
    sorted edge set and the state.  Every output and the workspace lie between guards, which must stay what they were, as must the
    inputs"""
    rows, dim = x.shape
    n = ctypes.c_size_t()
    H.call("ivit_linkage_workspace_bytes", rows, dim, splits, ctypes.byref(n))
    d_x, d_w = dev(x), dev(w)
    ws = Guarded(n.value)
    run = [Guarded(4 * rows), Guarded(rows), Guarded(4 * rows), Guarded(4 * rows), Guarded(4 * rows), Guarded(16)]
    args = (_P(d_x.data_ptr()), rows, dim, d_w is not None and _P(d_w.data_ptr()) or None, float(floor), splits, ws.ptr, n.value, *(g.ptr for g in run))
    state = lambda: run[5].payload().view(np.int32).copy()      # noqa: E731
    H.call("ivit_linkage_init", rows, *(g.ptr for g in run))
    assert state().tolist() == [rows, 1, 0, 0] and (run[2].payload().view(np.int32) == -1).all()
    while state()[1] != 0:                                 # the last round finds nothing to merge
        H.call("ivit_linkage_round", *args)
        assert state()[2] <= math.ceil(math.log2(rows))
    before = [g.payload().copy() for g in run]
    for _ in range(past):
        H.call("ivit_linkage_round", *args)
    torch.cuda.synchronize()
    assert all(np.array_equal(g.payload(), b) for g, b in zip(run, before)), "a round past the end wrote"
    assert all(g.guards_intact() for g in [ws] + run), "wrote outside an output"
    assert np.array_equal(d_x.cpu().numpy(), x) and (w is None or np.array_equal(d_w.cpu().numpy(), w)), "an input was written"
    u, v, val = run[2].payload().view(np.int32), run[3].payload().view(np.int32), run[4].payload().view(np.float32)
    assert np.array_equal(u < 0, v < 0) and not val[u < 0].view(np.uint32).any()            # the empty slots keep -1, -1, 0.0f
    order = np.lexsort((v[u >= 0], u[u >= 0], -val[u >= 0]))
    return [a[u >= 0][order] for a in (u, v, val)], state()


def test_linkage_entries_by_hand(H):
    x = blobs(300, 192, seed=2)
    w = inv_norms_reference(x)
    for floor in (-np.inf, 0.8):
        want = linkage_reference(x, w, floor)
        edges, state = by_hand(H, x, w, floor, splits=3, past=3)
        assert all(np.array_equal(a, b) for a, b in zip(edges, want)) and np.array_equal(edges[2].view(np.uint32), want[2].view(np.uint32))
        assert state[0] == 300 - len(want[0]) and state[1] == 0
        for splits in (1, 2, 7):
            assert all(np.array_equal(a, b) for a, b in zip(by_hand(H, x, w, floor, splits)[0], edges)), splits


def test_linkage_refusals(H):
    """each refused before anything is launched: every output and the workspace keep their fill"""
    x, rows, dim = dev(blobs(97, 64)), 97, 64
    n = ctypes.c_size_t()
    H.call("ivit_linkage_workspace_bytes", rows, dim, 2, ctypes.byref(n))
    arena = Guarded(n.value + 5 * 4 * rows + 16)
    ws = arena.ptr.value
    comp, u, v, val, done = (ws + n.value + 4 * rows * i for i in range(5))
    state = done + 4 * rows
    INV, UNS, lib = _lib.IVIT_ERR_INVALID, _lib.IVIT_ERR_UNSUPPORTED, H.lib
    err = lambda: lib.ivit_last_error(H.h)                  # noqa: E731

    def call(x_=x.data_ptr(), rows_=rows, dim_=dim, floor=0.5, splits=2, ws_=ws, bytes_=n.value, comp_=comp, state_=state):
        return lib.ivit_linkage_round(H.h, _P(x_), rows_, dim_, None, floor, splits, _P(ws_), bytes_, _P(comp_), _P(done), _P(u), _P(v), _P(val), _P(state_))

    init = lambda rows_=rows, comp_=comp, u_=u: lib.ivit_linkage_init(H.h, rows_, _P(comp_), _P(done), _P(u_), _P(v), _P(val), _P(state))      # noqa: E731
    assert call(dim_=96) == UNS and call(rows_=0) == INV and call(splits=65536) == INV
    assert call(state_=None) == INV and b"null" in err() and call(x_=None) == INV
    assert call(floor=float(np.nan)) == INV and b"floor" in err()
    assert call(bytes_=n.value - 1) == INV and b"workspace" in err()
    assert call(x_=x.data_ptr() + 4) == INV and b"x must be" in err() and call(comp_=comp + 2) == INV and b"comp must be" in err()
    assert call(comp_=x.data_ptr()) == INV and b"overlap" in err() and b"x" in err() and b"comp" in err()
    assert call(ws_=x.data_ptr()) == INV and b"overlap" in err()
    assert init(rows_=0) == INV and init(comp_=None) == INV and init(u_=comp) == INV and b"overlap" in err()
    assert lib.ivit_linkage_workspace_bytes(H.h, rows, 96, 0, ctypes.byref(n)) == UNS
    torch.cuda.synchronize()
    assert arena.untouched(), "a refused call wrote"
    assert init() == 0 and call(floor=float(-np.inf)) == 0 # and the same arguments, unharmed, are accepted
    torch.cuda.synchronize()
    assert arena.guards_intact() and not arena.untouched()


def test_linkage_run_captured_in_a_graph():
    """init and ceil(log2 rows) + 1 rounds in ONE graph: capture runs nothing; every replay leaves the eager edge set, on the captured
    rows and on new ones"""
    rows, dim = 300, 64
    stream = torch.cuda.Stream()
    h2 = _lib.Handle(0, stream.cuda_stream)
    n = ctypes.c_size_t()
    h2.call("ivit_linkage_workspace_bytes", rows, dim, 0, ctypes.byref(n))
    d, ws = dev(blobs(rows, dim)), torch.empty(n.value, dtype=torch.uint8, device="cuda")
    comp, u, v, state = (torch.empty(m, dtype=torch.int32, device="cuda") for m in (rows, rows, rows, 4))
    done, val = torch.empty(rows, dtype=torch.uint8, device="cuda"), torch.empty(rows, dtype=torch.float32, device="cuda")
    run = tuple(_P(t.data_ptr()) for t in (comp, done, u, v, val, state))

    def whole():
        h2.call("ivit_linkage_init", rows, *run)
        for _ in range(math.ceil(math.log2(rows)) + 1):
            h2.call("ivit_linkage_round", _P(d.data_ptr()), rows, dim, None, float(-np.inf), 0, _P(ws.data_ptr()), n.value, *run)

    with torch.cuda.stream(stream):
        whole()
    stream.synchronize()
    for t in (comp, u, v, state):
        t.fill_(-7)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
        whole()
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in (comp, u, v, state)), "the capture ran a launch"
    for x in (blobs(rows, dim), blobs(rows, dim, seed=5), chains(rows, 31, seed=2)[0]):
        d.copy_(dev(x))
        want = linkage_reference(x, None)
        with torch.cuda.stream(stream):
            whole()
        stream.synchronize()
        eager = [t.cpu().numpy().copy() for t in (comp, done, u, v, val, state)]
        assert eager[5][0] == 1 and eager[5][1] == 0 and int((eager[2] < 0).sum()) == 1
        for _ in range(2):
            u.fill_(-7)
            graph.replay()
            torch.cuda.synchronize()
            assert all(np.array_equal(t.cpu().numpy(), e) for t, e in zip((comp, done, u, v, val, state), eager))
        keep = eager[2] >= 0
        order = np.lexsort((eager[3][keep], eager[2][keep], -eager[4][keep]))
        assert all(np.array_equal(a[keep][order], b) for a, b in zip(eager[2:5], want))


@pytest.mark.parametrize("fname", ["micro_vit2h_b3.npz", "micro_swin_b2.npz"])
def test_linkage_fit_end_to_end(fname):
    cfg, eng = _engine(fname)
    images = torch.from_numpy(iv.make_images_int8(cfg, 12, seed=31)).cuda()
    batches = [images[:5], (torch.cat([images[5:], images[1:3]]).contiguous(), None)]       # rows 12 and 13 repeat images 1 and 2
    f8 = embed8(eng, batches)[0].cpu().numpy()
    tree, feat8 = linkage_fit(eng, batches)
    assert np.array_equal(feat8.cpu().numpy(), f8) and same(tree, linkage_reference(f8, inv_norms_reference(f8)))
    group = tree.cut(0.9999)
    assert group[12] == 1 and group[13] == 2 and tree.matrix().shape == (13, 4)
