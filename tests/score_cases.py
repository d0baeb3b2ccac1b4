"""Inputs that the CPU and the GPU tests of the score (rank and negative log-likelihood of the label, include/ivit_eval.h) share:
the tie, zero and rounding rows of test_predict_cpu.py::test_topk_reference_tie_and_zero_rules restated for the rank, a spread that
underflows exp, and the full-order statement of the rank."""
import numpy as np

INT32_MAX = 2 ** 31 - 1


def rule_rows():
    """[(name, acc int32 [n], scale float32 [n], order)]: `order` is the row's whole class order, so rank[order[j]] == j"""
    return [
        # one repeated value: ascending class index
        ("all equal", np.full(9, 7, np.int32), np.full(9, 0.25, np.float32), list(range(9))),
        # equal products from different pairs: 2 * 0.5 == 1 * 1.0 == 4 * 0.25
        ("equal products", np.array([1, 2, 0, 4, 3], np.int32), np.array([1.0, 0.5, 9.0, 0.25, 0.25], np.float32), [0, 1, 3, 4, 2]),
        # acc = 0 under a negative scale is -0.0: it ties +0.0 and the lower index wins
        ("signed zeros", np.array([-5, 0, 0, 0, -1], np.int32), np.array([1.0, -1.0, 1.0, -1.0, 1.0], np.float32), [1, 2, 3, 4, 0]),
        # int32 -> float32 is round-to-nearest-even: 2^24 + 1 -> 2^24, 2^24 + 3 -> 2^24 + 4, 2^31 - 1 -> 2^31
        ("rounding", np.array([2 ** 24 + 1, 2 ** 24 + 3, 2 ** 31 - 1, -2 ** 31], np.int64).astype(np.int32), np.ones(4, np.float32), [2, 1, 0, 3]),
    ]


def rule_batches():
    """every rule row once per class, labelled with that class -> [(name, acc [n, n], scale [n], labels [n], ranks [n])]"""
    out = []
    for name, acc, scale, order in rule_rows():
        n = len(acc)
        ranks = np.empty(n, np.int32)
        ranks[np.asarray(order)] = np.arange(n, dtype=np.int32)
        out.append((name, np.tile(acc, (n, 1)), scale, np.arange(n, dtype=np.int64), ranks))
    return out


def underflow_case():
    """values 0, -1000, -2000, 5: every exp but the maximum's (and class 0's, e^-5) underflows to zero, yet each nll is finite
    -> (acc [4, 4], scale [4], labels [4], nll [4] written out by hand)"""
    acc = np.tile(np.array([0, -1000, -2000, 5], np.int32), (4, 1))
    lse = np.log1p(np.exp(-5.0))                                     # log(e^0 + e^-5) above the maximum
    return acc, np.ones(4, np.float32), np.arange(4, dtype=np.int64), lse + np.array([5.0, 1005.0, 2005.0, 0.0])


def full_order_rank(acc, scale, labels):
    """the rank by its definition: the label's position in np.lexsort((arange(ncls), -(v + 0.0)))"""
    v = acc.astype(np.float32) * scale[None, :]
    cls = np.arange(acc.shape[1])
    return np.array([int(np.nonzero(np.lexsort((cls, -(row + np.float32(0.0)))) == l)[0][0]) for row, l in zip(v, labels)], np.int32)


def random_case(B, ncls, seed):
    """uniform int32 accumulators would put every nll near 1e5; these spread the values over a few tens, like a model's outputs,
    with scales of both signs as in the top-k tests -> (acc, scale, labels)"""
    rng = np.random.default_rng(seed)
    acc = rng.integers(-2 ** 20, 2 ** 20, size=(B, ncls), dtype=np.int64).astype(np.int32)
    scale = rng.uniform(1e-6, 1e-5, size=ncls).astype(np.float32)
    scale[rng.random(ncls) < 0.3] *= -1
    return acc, scale, rng.integers(0, ncls, size=B).astype(np.int64)
