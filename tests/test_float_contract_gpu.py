"""ivit_logreg_loss_grad (include/ivit_logreg.h), ivit_gauss_prepare and ivit_gauss_score (include/ivit_gauss.h) on the arena harness of
tests/abi_cases.py, as tests/test_views_gpu.py runs the view entries: every array in its own [1 MiB guard | payload | 1 MiB guard]
allocation.  No byte lands in front of or behind an output or the workspace and every documented output byte is written; the outputs
are the same bytes with 0x7F and with 0xFF around the inputs (both score kernels clamp their last rows and prefetch past their part's
last step); every pointer moved by one element is refused with the header's message or gives the same bytes; every output laid over an
input or another output is refused with both names; the captured-graph contract holds with a second set of contents.

The workspace is an output of which no byte is pinned, sized by the entry's own size query."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import abi_cases as A  # noqa: E402
import float_cases as F  # noqa: E402
from ivit_amd import _lib, gauss  # noqa: E402
from ivit_amd.probe import logreg_loss_grad  # noqa: E402

ROWS = F.CONTRACT_TILE_ROWS
ARGNAMES = {name: [p.name for p in abi.functions[name].params[1:]] for abi in (_lib.LOGREG_ABI, _lib.GAUSS_ABI) for name in abi.functions}
I, O = A._io()

# What happens when ONE pointer is moved forward by one element, from the REQUIRE_A16 / REQUIRE_ALIGNED lines of the three launchers
# (csrc/ivit_hip.hip); the indices are the arguments', handle not counted.  The arrays of 4- and 8-byte elements that need only their
# element's alignment are touched with element-sized accesses alone (labels[row], b[c], grad_b[i], loss[0], correct[0 .. 1]; t[r] and
# bc[c] in gauss_prepare_kernel; q, best, cls and dist one element per thread in gauss_finish_kernel), so one element further they give
# the same bytes; the 16-byte-aligned ones are loaded or stored 16 bytes per lane and are refused.  The workspace and the prepared model
# are byte arrays here: one element is one byte.
ALIGN = {
    "ivit_logreg_loss_grad": {0: A._a16("feat8"), 1: "exact", 4: A._a16("W"), 5: "exact", 9: A._a16("workspace"), 11: "exact", 12: A._a16("grad_W"),
                              13: "exact", 14: "exact"},
    "ivit_gauss_prepare": {0: A._a16("Wh"), 1: "exact", 2: A._a16("Wc"), 3: "exact", 7: A._a16("model")},
    "ivit_gauss_score": {0: A._a16("model"), 2: A._a16("feat8"), 8: A._a16("workspace"), 10: "exact", 11: "exact", 12: "exact", 13: "exact"},
}
INPUTS = {"ivit_logreg_loss_grad": (0, 1, 4, 5), "ivit_gauss_prepare": (0, 1, 2, 3), "ivit_gauss_score": (0, 2)}


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


def _size(fn, *args):
    n = ctypes.c_size_t(0)
    assert fn(*args, ctypes.byref(n)) == 0
    return n.value


def _workspace(nbytes):
    return O(np.zeros(nbytes, np.uint8), ("free", np.zeros(nbytes, bool)))


def logreg_args(H, N, C, dim, splits, seed=0):
    x, lab, W, b, s = F.logreg_case(N, C, dim, seed)
    nbytes = _size(H.lib.ivit_logreg_workspace_bytes, N, dim, C, splits)
    return [I(x), I(lab), N, dim, I(W), I(b), C, s, splits, _workspace(nbytes), nbytes, O(np.zeros(1, np.float64)), O(np.zeros((C, dim), np.float32)),
            O(np.zeros(C, np.float32)), O(np.zeros(2, np.int64))]


def prepare_args(H, N, dim, R, C, seed=0):
    x, Wh, t, Wc, bc = F.gauss_arrays(N, dim, R, C, seed)
    bc[C // 2] = -np.inf                                            # an empty class beside the padding rows' -inf
    nbytes = _size(H.lib.ivit_gauss_model_bytes, dim, R, C)
    return x, [I(Wh), I(t), I(Wc), I(bc), dim, R, C, O(np.zeros(nbytes, np.uint8)), nbytes]


def score_args(H, N, dim, R, C, splits, seed=0):
    """the prepared model is the bytes ivit_gauss_prepare wrote on plain allocations"""
    x, pargs = prepare_args(H, N, dim, R, C, seed)
    model = A.plain_outputs(H.lib.ivit_gauss_prepare, H.h, pargs, A.TorchMem())[0]
    nbytes = _size(H.lib.ivit_gauss_workspace_bytes, N, dim, R, C, splits)
    out = lambda dtype: O(np.zeros(N, dtype))
    return [I(model), model.size, I(x), N, dim, R, C, splits, _workspace(nbytes), nbytes, out(np.float32), out(np.float32), out(np.int32), out(np.float32)]


def _contract(H, name, args, args2):
    """checks 1 and 2, the plain call, every pointer one element off, every overlap, the stream and graph contract -> the outputs"""
    fn, mem = getattr(H.lib, name), A.TorchMem()
    got = A.check_contract(fn, H.h, args, mem, what=name, tile_rows=ROWS)
    plain = A.plain_outputs(fn, H.h, args, mem)
    assert len(got) == len(plain) and all(np.array_equal(g, p) for g, p in zip(got, plain))
    arrays = [i for i, a in enumerate(args) if A._is_array(a)]
    assert sorted(ALIGN[name]) == arrays                            # every pointer of the entry has its recorded outcome
    for idx, outcome in ALIGN[name].items():
        A.check_alignment(fn, H, args, mem, None, idx, outcome, got, name, tile_rows=ROWS)
    A.check_overlap(fn, H, args, mem, None, name, tile_rows=ROWS, inplace={}, inputs=INPUTS[name], argnames=ARGNAMES[name])
    want1, want2 = A.check_stream_contract(fn, H, args, args2, mem, what=name)
    assert all(np.array_equal(a, b) for a, b in zip(want1, got)) and any(not np.array_equal(a, b) for a, b in zip(want1, want2))
    return got


@pytest.mark.parametrize("N,C,dim,splits", F.LOGREG_CONTRACT_CASES, ids=str)
def test_logreg_loss_grad_contract(H, N, C, dim, splits):
    args = logreg_args(H, N, C, dim, splits)
    got = _contract(H, "ivit_logreg_loss_grad", args, logreg_args(H, N, C, dim, splits, seed=1))
    dev = [torch.from_numpy(a[1]).cuda() for a in (args[0], args[1], args[4], args[5])]
    want = [t.cpu().numpy() for t in logreg_loss_grad(*dev, args[7], splits)]                  # the product path: the same bits
    assert all(np.array_equal(g, w.view(np.uint8).reshape(-1)) for g, w in zip(got[1:], want))


@pytest.mark.parametrize("N,dim,R,C,splits", F.GAUSS_CONTRACT_CASES, ids=str)
def test_gauss_prepare_contract(H, N, dim, R, C, splits):
    _, args = prepare_args(H, N, dim, R, C)
    got = _contract(H, "ivit_gauss_prepare", args, prepare_args(H, N, dim, R, C, seed=1)[1])
    m = gauss.GaussModel(*(a[1] for a in args[:4]))
    assert np.array_equal(got[0], m.prepared("cuda")[1].cpu().numpy())


@pytest.mark.parametrize("N,dim,R,C,splits", F.GAUSS_CONTRACT_CASES, ids=str)
def test_gauss_score_contract(H, N, dim, R, C, splits):
    args = score_args(H, N, dim, R, C, splits)
    got = _contract(H, "ivit_gauss_score", args, score_args(H, N, dim, R, C, splits, seed=1))
    x, pargs = prepare_args(H, N, dim, R, C)
    dist, cls, q, best = (t.cpu().numpy() for t in gauss.score(torch.from_numpy(x).cuda(), gauss.GaussModel(*(a[1] for a in pargs[:4])), splits))
    assert all(np.array_equal(g, w.view(np.uint8).reshape(-1)) for g, w in zip(got[1:], (q, best, cls, dist)))
