"""ivit_gauss_score (include/ivit_gauss.h) against predict.gauss_score_reference: the shapes at which the scorer changes its path, equal
scores in two tiles, -inf classes, the same bits for every `splits`, call and graph replay, the refusals, and engine.novelty; every
width the launcher dispatches on, and one-hot models whose four outputs are known bit for bit (tests/float_cases.py)."""
import ctypes

import numpy as np
import pytest

from conftest import golden_scales, load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import float_cases as F  # noqa: E402
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib, gauss  # noqa: E402
from ivit_amd.predict import gauss_score_reference  # noqa: E402

# The accuracy rule: the entry may not be further from the float64 reference than the plain fp32 torch route (feat8.float() @ Wh.T + t,
# squares summed; @ Wc.T + bc, max) is, with a factor 2 for another order of summation.  Measured on an MI355X over SHAPES with `case`'s
# data (tools/gauss_bench.py --errors; profiles/README.md, "Novelty scores"): the torch route's largest |q - q64| / max q64 is
# TORCH_Q_ERR and its largest |best - best64| / max |s64| TORCH_BEST_ERR; the bounds are twice that, and dist is held to the sum of the
# two absolute bounds.
TORCH_Q_ERR, TORCH_BEST_ERR = 1.777e-7, 6.761e-7         # the entry's own on that run: 2.087e-7 and 3.298e-7
Q_BOUND, BEST_BOUND = 2 * TORCH_Q_ERR, 2 * TORCH_BEST_ERR

# (N, dim, R, C, splits).  N: below, around and across the 128-row block, a ragged last 32-row step; dim: the smallest (KS = 1: a step
# of the scorer is a whole tile, three wavefronts per SIMD), 128 (the first whose tiles span two steps; two wavefronts), 192, 448 and
# 512 (the last with two wavefronts per SIMD and the first with one), the largest; R: one tile, three, all of dim; C: one class, a
# partial second tile, three tiles; splits: the library's, one part, three (more than the two tiles of R = 32, C = 1)
SHAPES = [(1, 64, 32, 1, 3), (127, 192, 96, 33, 1), (129, 64, 64, 70, 0), (300, 192, 192, 70, 3), (300, 1024, 96, 33, 0), (129, 1024, 1024, 1, 1),
          (127, 64, 32, 70, 0), (300, 1024, 32, 70, 3), (1, 192, 32, 33, 1), (129, 128, 128, 33, 3), (300, 128, 96, 1, 0), (127, 192, 192, 1, 3),
          (129, 448, 96, 70, 0), (300, 512, 512, 33, 1)]


def case(N, dim, R, C, seed=0):
    """x and a model whose q and scores are of unit-to-R size: one generator for the suites and tools/gauss_bench.py"""
    x, *model = F.gauss_arrays(N, dim, R, C, seed)
    return x, gauss.GaussModel(*model)


def run(x, model, splits=0):
    return [t.cpu().numpy() for t in gauss.score(torch.from_numpy(x).cuda(), model, splits)]


def reference(x, m):
    dist, cls, q, best = gauss_score_reference(x, m.Wh, m.t, m.Wc, m.bc)
    s = x.astype(np.float64) @ m.Wc.astype(np.float64).T + m.bc.astype(np.float64)
    top = np.sort(s, axis=1)
    return dist, cls, q, best, np.abs(s).max(), top[:, -1] - top[:, -2] if s.shape[1] > 1 else np.full(len(x), np.inf)


def check(got, want, q_bound=Q_BOUND, best_bound=BEST_BOUND):
    dist, cls, q, best = got
    wd, wc, wq, wb, smax, gap = want
    print("q err %.3e  best err %.3e  dist abs err %.3e" % (np.abs(q - wq).max() / wq.max(), np.abs(best - wb).max() / smax, np.abs(dist - wd).max()))
    clear = gap > 1e-5 * smax
    assert clear.mean() >= 0.99 and np.array_equal(cls[clear], wc[clear]) and cls.dtype == np.int32
    assert np.abs(q - wq).max() <= q_bound * wq.max() and np.abs(best - wb).max() <= best_bound * smax
    assert np.abs(dist - wd).max() <= q_bound * wq.max() + best_bound * smax


@pytest.mark.parametrize("N,dim,R,C,splits", SHAPES)
def test_entry_equals_the_reference(N, dim, R, C, splits):
    x, model = case(N, dim, R, C)
    check(run(x, model, splits), reference(x, model))


# Every width the launcher dispatches on (tests/float_cases.py), under the same rule with the torch route's error measured on THESE
# cases (tools/gauss_bench.py --errors on an MI355X; profiles/README.md, "Novelty scores", "Every width and one-hot models"):
# (TORCH_Q_ERR, TORCH_BEST_ERR) of the list, the bounds twice that.
WIDTH_TORCH_ERR = (4.558e-7, 9.746e-7)   # the entry's own on that run: 1.939e-7 and 2.677e-7


def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


@pytest.mark.parametrize("N,dim,R,C,splits,seed", F.GAUSS_WIDTH_CASES, ids=_ids(F.GAUSS_WIDTH_CASES))
def test_every_dispatched_width_equals_the_reference(N, dim, R, C, splits, seed):
    """gauss_score_kernel<KS>, KS = dim / 64 = 1 .. 16; R = dim at the widths of the workload's own backbones"""
    x, model = case(N, dim, R, C, seed)
    check(run(x, model, splits), reference(x, model), 2 * WIDTH_TORCH_ERR[0], 2 * WIDTH_TORCH_ERR[1])


@pytest.mark.parametrize("dim,R,splits", F.ONEHOT_GAUSS_CASES, ids=_ids(F.ONEHOT_GAUSS_CASES))
def test_one_hot_models_bit_for_bit(dim, R, splits):
    """one nonzero weight per table row (24 significant bits, exponents 2^-30 .. 2^30 inside a tile), features that are powers of
    two: every z and s is one exact product whatever order the matrix instruction adds in, and the header's order fixes q, so all
    four outputs are known to the bit.  A weight in the wrong place of the prepared layout, a lost piece, a piece scaled wrongly or
    a class index off by a half moves at least one of them"""
    x, *model = F.onehot_case(dim, R)
    want = F.onehot_gauss_expected(x, *model)
    got = run(np.array(x), gauss.GaussModel(*(np.array(a) for a in model)), splits)      # copies: the case's arrays are read-only
    for name, g, w in zip(("dist", "cls", "q", "best"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, int((g != w).sum()), "elements differ")


def test_equal_largest_scores_in_two_tiles_take_the_smaller_index():
    x, m = case(127, 64, 32, 70, seed=3)
    m.Wc[40], m.bc[40] = m.Wc[3], 50.0
    m.bc[3] = 50.0                                                # classes 3 and 40: the same bits, above every other score, in two tiles
    for splits in (0, 1):
        assert (run(x, m, splits)[1] == 3).all()


def test_minus_infinity_classes_are_never_chosen_and_make_no_nan():
    x, m = case(129, 192, 96, 33, seed=4)
    m.bc[[0, 5, 32]] = -np.inf
    dist, cls, q, best = run(x, m)
    wd, wc = gauss_score_reference(x, m.Wh, m.t, m.Wc, m.bc)[:2]
    assert not np.isin(cls, [0, 5, 32]).any() and np.isfinite(dist).all() and (cls == wc).mean() >= 0.99
    m = gauss.GaussModel(m.Wh, m.t, m.Wc, np.full(33, -np.inf, np.float32))
    dist, cls, q2, best = run(x, m, 3)
    assert (cls == 0).all() and (best == -np.inf).all() and (dist == np.inf).all() and np.array_equal(q2, q)


def test_every_splits_a_second_call_and_a_captured_graph_give_the_same_bits():
    x, m = case(300, 192, 96, 70, seed=5)
    xd = torch.from_numpy(x).cuda()
    eager = [t.cpu().numpy() for t in gauss.score(xd, m, 1)]
    for splits in (3, 0, 1):
        assert all(np.array_equal(t.cpu().numpy(), e) for t, e in zip(gauss.score(xd, m, splits), eager)), splits
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
        out = gauss.score(xd, m, 3)
    for _ in range(3):
        for t in out:
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(t.cpu().numpy(), e) for t, e in zip(out, eager))


def test_refusals_launch_nothing():
    x, m = case(64, 128, 64, 33, seed=6)
    xd = torch.from_numpy(x).cuda()
    H, model = m.prepared(xd.device)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    n = ctypes.c_size_t(0)
    assert H.lib.ivit_gauss_workspace_bytes(64, 128, 64, 33, 0, ctypes.byref(n)) == 0
    for dim, R, status in ((96, 64, _lib.IVIT_ERR_UNSUPPORTED), (128, 48, _lib.IVIT_ERR_INVALID), (128, 160, _lib.IVIT_ERR_INVALID)):
        assert H.lib.ivit_gauss_workspace_bytes(64, dim, R, 33, 0, ctypes.byref(n)) == status
        assert H.lib.ivit_gauss_model_bytes(dim, R, 33, ctypes.byref(n)) == status
    odd = torch.zeros(64 * 128 + 16, dtype=torch.int8, device="cuda")[1:1 + 64 * 128].view(64, 128)
    with pytest.raises(_lib.IvitError, match="feat8 must be 16-byte aligned"):
        gauss.score(odd, m)
    ws, q, best, cls, dist = (torch.full((k,), 7, dtype=torch.uint8, device="cuda") for k in (n.value, 256, 256, 256, 256))
    before = model.clone()
    for over, name in ((xd, "feat8"), (model, "model")):          # dist laid over an input
        st = H.lib.ivit_gauss_score(H.h, P(model), model.numel(), P(xd), 64, 128, 64, 33, 0, P(ws), n.value, P(q), P(best), P(cls), P(over))
        err = H.lib.ivit_last_error(H.h).decode()
        assert st == _lib.IVIT_ERR_INVALID and "overlap" in err and "dist" in err and name in err, err
    for dim, R, status in ((96, 64, _lib.IVIT_ERR_UNSUPPORTED), (128, 48, _lib.IVIT_ERR_INVALID), (128, 160, _lib.IVIT_ERR_INVALID)):
        st = H.lib.ivit_gauss_score(H.h, P(model), model.numel(), P(xd), 64, dim, R, 33, 0, P(ws), n.value, P(q), P(best), P(cls), P(dist))
        assert st == status
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in (ws, q, best, cls, dist)) and torch.equal(model, before) and np.array_equal(xd.cpu().numpy(), x)


def test_engine_novelty_equals_features_then_score():
    from ivit_amd.engine import ViTEngine
    g = load_golden("micro_vit_b2.npz")
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    eng = ViTEngine.from_float(cfg, iv.make_vit_weights(cfg, int(g["seed"])), golden_scales(g))
    images = torch.from_numpy(iv.make_images_int8(cfg, 9, seed=3)).cuda()
    feat8 = eng.features(images, copy=True)[0]
    m = case(1, eng.num_features, 32, 5, seed=7)[1]
    want = gauss.score(feat8, m)
    dist, cls, f = eng.novelty(images, m, copy=True)
    assert torch.equal(dist, want[0]) and torch.equal(cls, want[1]) and torch.equal(f, feat8) and bool(torch.isfinite(dist).all())
