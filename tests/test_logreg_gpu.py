"""ivit_logreg_loss_grad (include/ivit_logreg.h) against predict.logreg_reference: the shapes at which the two kernels change their path,
ignored rows, logits of +-80, equal logits, determinism, a captured graph, the refusals, and fit_logistic end to end; then the case
lists of tests/float_cases.py: every width the launcher dispatches on, both sides of the part-length limit, one-hot weights."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import float_cases as F  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from ivit_amd.predict import logreg_reference  # noqa: E402
from ivit_amd.probe import fit_logistic, logreg_loss_grad  # noqa: E402

# The accuracy rule: the entry may not be further from the float64 reference than the plain fp32 torch route (feat8.float() @ W.T,
# softmax, matmul) is, with a factor 2 for another order of summation.  Measured on an MI355X over SHAPES with `case`'s data
# (tools/logreg_bench.py --errors; profiles/README.md, "Logistic probe"): the torch route's largest error is TORCH_GRAD_ERR relative
# to max|grad| (grad_W and grad_b alike) and TORCH_LOSS_ERR relative for the loss, over SHAPES and the two further cases below that
# `check` judges (labels outside the range, logits of +-80); the bounds are twice that.
TORCH_GRAD_ERR, TORCH_LOSS_ERR = 5.761e-7, 1.647e-7      # the entry's own on that run: 2.165e-7 and 1.647e-7 (three bf16 pieces a side)
GRAD_BOUND, LOSS_BOUND = 2 * TORCH_GRAD_ERR, 2 * TORCH_LOSS_ERR

# (N, C, dim, splits).  N: below, around and across the 128-row tile of the row pass, a ragged last 32-row step; C: one partial class
# tile, a full tile and one class, three tiles; dim: the smallest (two wavefronts of the gradient pass idle), one whose feature tiles
# split unevenly over the wavefronts, the largest; splits: the library's, one part, three
SHAPES = [(1, 2, 64, 0), (127, 2, 192, 1), (129, 33, 64, 3), (300, 70, 192, 0), (300, 33, 1024, 1), (129, 70, 1024, 3), (127, 70, 64, 0),
          (300, 2, 1024, 3), (1, 33, 192, 1), (129, 2, 64, 1), (300, 70, 64, 3), (127, 33, 192, 0)]


case = F.logreg_case      # x, labels, W, b, x_scale with logits of about unit size: one generator for the suites and tools/logreg_bench.py


def run(x, lab, W, b, s, splits=0):
    out = logreg_loss_grad(torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda(), torch.from_numpy(W).cuda(), torch.from_numpy(b).cuda(), s, splits)
    return [t.cpu().numpy() for t in out]


def check(got, want, grad_bound=GRAD_BOUND, loss_bound=LOSS_BOUND):
    loss, gW, gb, correct = got
    print("loss rel err %.3e  grad_W err %.3e  grad_b err %.3e" % (abs(loss[0] - want[0]) / max(abs(want[0]), 1e-300),
          np.abs(gW - want[1]).max() / np.abs(want[1]).max(), np.abs(gb - want[2]).max() / np.abs(want[2]).max()))
    assert np.array_equal(correct, want[3])
    assert abs(loss[0] - want[0]) <= loss_bound * abs(want[0])
    assert np.abs(gW - want[1]).max() <= grad_bound * np.abs(want[1]).max() and np.abs(gb - want[2]).max() <= grad_bound * np.abs(want[2]).max()


@pytest.mark.parametrize("N,C,dim,splits", SHAPES)
def test_entry_equals_the_reference(N, C, dim, splits):
    x, lab, W, b, s = case(N, C, dim)
    check(run(x, lab, W, b, s, splits), logreg_reference(x, lab, W, b, s))


@pytest.mark.parametrize("every", [False, True])
def test_rows_with_labels_outside_the_range_count_for_nothing(every):
    x, lab, W, b, s = case(300, 33, 192, seed=1)
    lab[::3] = np.array([-1, 33, 2 ** 31 - 1, -2 ** 31])[np.arange(100) % 4]
    if every:
        lab[:] = 33
    loss, gW, gb, correct = run(x, lab, W, b, s)
    want = logreg_reference(x, lab, W, b, s)
    assert np.array_equal(correct, want[3]) and correct[0] == (0 if every else 200)
    if every:
        assert loss[0] == 0 and not gW.any() and not gb.any() and correct.tolist() == [0, 0]
    else:
        check((loss, gW, gb, correct), want)


def test_logits_of_plus_and_minus_80_do_not_overflow():
    x, lab, W, b, s = case(129, 33, 192, seed=2)
    x[7] = -128
    W[0], W[1] = 80 / (s * 128 * 192), -80 / (s * 128 * 192)      # row 7: z[0] = -80, z[1] = +80 beside unit logits
    b[:2] = 0
    want = logreg_reference(x, lab, W, b, s)
    got = run(x, lab, W, b, s, 1)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    check(got, want)


def test_equal_largest_logits_take_the_smaller_index():
    x, lab, W, b, s = case(127, 70, 64, seed=3)
    W[40], b[40] = W[3], 50.0
    b[3] = 50.0                                                   # classes 3 and 40: the same bits, above every other logit, in two tiles
    lab[:] = np.where(np.arange(127) % 2, 3, 40)
    correct = run(x, lab, W, b, s)[3]
    assert correct.tolist() == [127, 63] == logreg_reference(x, lab, W, b, s)[3].tolist()


def test_two_calls_and_a_captured_graph_give_the_same_bits():
    x, lab, W, b, s = case(300, 70, 192, seed=4)
    dev = [torch.from_numpy(a).cuda() for a in (x, lab, W, b)]
    eager = [t.cpu().numpy() for t in logreg_loss_grad(*dev, s, 3)]
    again = [t.cpu().numpy() for t in logreg_loss_grad(*dev, s, 3)]
    assert all(np.array_equal(a, e) for a, e in zip(again, eager))
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
        out = logreg_loss_grad(*dev, s, 3)
    for _ in range(3):
        for t in out:
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(t.cpu().numpy(), e) for t, e in zip(out, eager))


def test_refusals_launch_nothing():
    x, lab, W, b, s = case(64, 33, 128, seed=5)
    xd, ld, Wd, bd = (torch.from_numpy(a).cuda() for a in (x, lab, W, b))
    with pytest.raises(_lib.IvitError):                           # dim = 96
        logreg_loss_grad(xd[:, :96].contiguous(), ld, Wd[:, :96].contiguous(), bd, s)
    with pytest.raises(_lib.IvitError):                           # C = 1
        logreg_loss_grad(xd, ld, Wd[:1], bd[:1], s)
    odd = torch.zeros(64 * 128 + 16, dtype=torch.int8, device="cuda")[1:1 + 64 * 128].view(64, 128)
    with pytest.raises(_lib.IvitError, match="feat8 must be 16-byte aligned"):
        logreg_loss_grad(odd, ld, Wd, bd, s)
    H, P = _lib.Handle(0, torch.cuda.current_stream().cuda_stream), lambda t: ctypes.c_void_p(t.data_ptr())
    n = ctypes.c_size_t(0)
    assert H.lib.ivit_logreg_workspace_bytes(64, 128, 33, 0, ctypes.byref(n)) == 0
    ws, loss, gb, cor = (torch.full((k,), 7, dtype=torch.uint8, device="cuda") for k in (n.value, 8, 33 * 4, 16))
    st = H.lib.ivit_logreg_loss_grad(H.h, P(xd), P(ld), 64, 128, P(Wd), P(bd), 33, s, 0, P(ws), n.value, P(loss), P(Wd), P(gb), P(cor))
    err = H.lib.ivit_last_error(H.h).decode()
    assert st == _lib.IVIT_ERR_INVALID and "overlap" in err and "grad_W" in err and "W" in err
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in (ws, loss, gb, cor)) and np.array_equal(Wd.cpu().numpy(), W)


def test_fit_logistic_classifies_as_the_float64_reference_fit():
    rng = np.random.default_rng(6)
    lab = rng.integers(5, size=600)
    x = np.clip(rng.integers(-30, 31, size=(5, 192))[lab] + rng.integers(-60, 61, size=(600, 192)), -128, 127).astype(np.int8)
    ref = fit_logistic(x, lab, 5, 0.02, l2=1e-3, iters=100, evaluate=logreg_reference)
    pred = ref.logits_reference(x).argmax(axis=1)
    zf = np.float64(np.float32(0.02)) * x.astype(np.float64) @ ref.weight.astype(np.float64).T + ref.bias
    assert (pred == zf.argmax(axis=1)).mean() >= 0.99             # the int8 head of the reference fit against its own float weights
    xd, ld = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()
    head = fit_logistic([xd[:250], xd[250:]], ld, 5, 0.02, l2=1e-3, iters=100)
    assert (head.logits_reference(x).argmax(axis=1) == pred).mean() >= 0.99


# ---------------------------------------------------------------- the case lists of tests/float_cases.py
# The accuracy rule on three further lists, each with the torch route's error measured on ITS cases (tools/logreg_bench.py --errors on
# an MI355X; profiles/README.md, "Logistic probe", "Every width, both sides of the part limit, one-hot models"): (TORCH_GRAD_ERR,
# TORCH_LOSS_ERR) of the list, the bounds twice that.  As above, the gradient figure is the larger of the torch route's two (grad_W).
WIDTH_TORCH_ERR = (5.761e-7, 6.489e-8)   # every width: the entry's own on that run: 1.728e-7 (grad_b 1.652e-7) and 2.135e-8
FLUSH_TORCH_ERR = (2.171e-6, 6.945e-8)   # both sides of LOGREG_FLUSH_ROWS: the entry's own: 8.587e-7 (grad_b 3.074e-7) and 1.352e-8
ONEHOT_TORCH_ERR = (0.0, 5.557e-8)       # one-hot models: every gradient is an exact integer on both routes; the entry's loss: 6.255e-9


def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


@pytest.mark.parametrize("N,C,dim,splits,seed", F.LOGREG_WIDTH_CASES, ids=_ids(F.LOGREG_WIDTH_CASES))
def test_every_dispatched_width_equals_the_reference(N, C, dim, splits, seed):
    """logreg_rows_kernel<KS>, KS = dim / 64 = 1 .. 16, and logreg_grad_kernel<NT>, NT = 1 .. 8 (two widths each: the feature tiles
    split evenly over the four wavefronts at one, unevenly at the other)"""
    x, lab, W, b, s = case(N, C, dim, seed)
    check(run(x, lab, W, b, s, splits), logreg_reference(x, lab, W, b, s), 2 * WIDTH_TORCH_ERR[0], 2 * WIDTH_TORCH_ERR[1])


def _workspace_bytes(N, dim, C, splits):
    n = ctypes.c_size_t(0)
    assert _lib.load().ivit_logreg_workspace_bytes(N, dim, C, splits, ctypes.byref(n)) == 0
    return n.value


@pytest.mark.parametrize("N,C,dim,splits,seed", F.LOGREG_FLUSH_CASES, ids=_ids(F.LOGREG_FLUSH_CASES))
def test_both_sides_of_the_part_length_limit(N, C, dim, splits, seed):
    """a part of the gradient pass holds at most LOGREG_FLUSH_ROWS rows whatever `splits` asks for: 65536 rows are one part, 65537
    with splits = 1 two of 32800 and 32737 (ragged), and the size query states at least what the device's layout needs
    (float_cases.logreg_layout: the launcher's arithmetic restated; tests/test_float_cases_cpu.py checks it without a device)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    dev, most = F.logreg_layout(N, dim, C, splits, cus), F.logreg_layout(N, dim, C, splits, 0)
    assert dev["per"] <= F.LOGREG_FLUSH_ROWS and dev["per"] % 32 == 0 and (dev["parts"] - 1) * dev["per"] < N <= dev["parts"] * dev["per"]
    assert (dev["parts"] == 1) == (N <= F.LOGREG_FLUSH_ROWS)
    if splits == 1:
        assert (dev["parts"], dev["per"]) == ((1, 65536) if N == 65536 else (2, 32800))
    assert _workspace_bytes(N, dim, C, splits) == most["bytes"] >= dev["bytes"]
    x, lab, W, b, s = case(N, C, dim, seed)
    check(run(x, lab, W, b, s, splits), logreg_reference(x, lab, W, b, s), 2 * FLUSH_TORCH_ERR[0], 2 * FLUSH_TORCH_ERR[1])


@pytest.mark.parametrize("dim,splits", F.ONEHOT_LOGREG_CASES, ids=_ids(F.ONEHOT_LOGREG_CASES))
def test_one_hot_weights_give_exact_logits(dim, splits):
    """one nonzero weight per class, 24 significant bits each, exponents 2^-30 .. 2^30 inside a class tile, features that are powers
    of two: every logit is one exact product, so `correct` has no tolerance (check asserts it exactly) whatever piece or exponent a
    kernel mishandles; loss and gradient under the accuracy rule"""
    x, lab, W, b, s = (np.array(a) if isinstance(a, np.ndarray) else a for a in F.onehot_logreg_case(dim))
    want = logreg_reference(x, lab, W, b, s)
    assert 0 < want[3][1] < want[3][0] == len(x)
    check(run(x, lab, W, b, s, splits), want, 2 * ONEHOT_TORCH_ERR[0], 2 * ONEHOT_TORCH_ERR[1])
