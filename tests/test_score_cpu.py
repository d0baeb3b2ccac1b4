"""The score without a GPU: include/ivit_eval.h declares the five entries, they are bound under names of their own and exported
while ivit.h and its binding stay what they were, both kernel forms are in the gfx950 code object, `score_reference` states the
contract (rank in the top-k's order, fp64 negative log-likelihood, the out-of-range rule), and `evaluate(loss=True)` counts what
`evaluate` counts and averages the loss — ragged batches, a top-16 on 10 classes, a bad label, no batches, two gloo ranks."""
import glob
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden
import ivit_amd as iv
from ivit_amd import _abi, _lib
from score_cases import INT32_MAX, full_order_rank, random_case, rule_batches, underflow_case
from test_predict_cpu import StubEngine, _batches, _device_code_object, _eval_case, _free_port

ENTRIES = {"ivit_logits_score": 8, "ivit_vit_score": 11, "ivit_swin_score": 11, "ivit_vit_score_graph_create": 12,
           "ivit_swin_score_graph_create": 12}


# ---------------------------------------------------------------- the second header and its binding
def test_eval_header_declares_score_entries():
    hdr = open(os.path.join(ROOT, "include", "ivit_eval.h")).read()
    assert re.search(r'#include "ivit\.h"', hdr) and "quant_train.py:335-339" in hdr
    assert int(re.search(r"#define IVIT_EVAL_VERSION (\d+)", hdr).group(1)) == 1 == _lib.IVIT_EVAL_VERSION
    outs = r"int32_t\s*\*\s*rank\s*,\s*double\s*\*\s*nll"
    assert re.search(r"int\s+ivit_logits_score\s*\(\s*ivit_handle\s+h\s*,\s*const\s+int32_t\s*\*\s*logits\s*,\s*const\s+float\s*\*\s*scale\s*,"
                     r"\s*const\s+int64_t\s*\*\s*labels\s*,\s*int\s+batch\s*,\s*int\s+num_classes\s*,\s*" + outs + r"\s*\)", hdr)
    tail = (r"const\s+int8_t\s*\*\s*images\s*,\s*int\s+batch\s*,\s*int\s+nslices\s*,\s*void\s*\*\s*workspace\s*,\s*size_t\s+bytes\s*,"
            r"\s*int32_t\s*\*\s*logits\s*,\s*const\s+float\s*\*\s*head_scale\s*,\s*const\s+int64_t\s*\*\s*labels\s*,\s*" + outs)
    for kind in ("vit", "swin"):
        assert re.search(rf"int\s+ivit_{kind}_score\s*\(\s*ivit_{kind}\s+m\s*,\s*{tail}\s*\)", hdr), kind
        assert re.search(rf"int\s+ivit_{kind}_score_graph_create\s*\(\s*ivit_{kind}\s+m\s*,\s*{tail}\s*,\s*ivit_graph\s*\*\s*out\s*\)", hdr), kind


def test_score_entries_bound_and_exported_beside_an_unchanged_ivit_h():
    iv.build()
    lib = _lib.load()
    P, I = _lib._P, _lib._I
    assert list(_abi.EVAL_ABI.functions) == list(ENTRIES) == list(_lib.EVAL_SIGNATURES) == list(_lib.EVAL_RESTYPES)
    for name, nparams in ENTRIES.items():
        bound = getattr(lib, name)
        assert len(_lib.EVAL_SIGNATURES[name]) == nparams and bound.argtypes == _lib.EVAL_SIGNATURES[name] and bound.restype is I, name
    assert _lib.EVAL_SIGNATURES["ivit_logits_score"] == [P, P, P, P, I, I, P, P]
    assert _lib.EVAL_SIGNATURES["ivit_vit_score"] == [P, P, I, I, P, __import__("ctypes").c_size_t, P, P, P, P, P]
    assert _abi.EVAL_ABI.constants == {"IVIT_EVAL_VERSION": 1}
    # ivit.h and what is derived from it: 99 prototypes, version 111, none of the new names
    hdr = open(os.path.join(ROOT, "include", "ivit.h")).read()
    assert len(_lib.ABI.functions) == 99 and set(_lib.SIGNATURES) == set(_lib.ABI.functions) and _lib.IVIT_VERSION == 111
    assert not set(ENTRIES) & set(_lib.SIGNATURES) and "_score" not in hdr and "ivit_eval.h" not in hdr
    assert _abi.parse(hdr).functions.keys() == _lib.ABI.functions.keys()
    # a header that names a handle of ivit.h parses only with ivit.h as its base
    with pytest.raises(_abi.AbiError):
        _abi.parse(open(_abi.EVAL_HEADER).read())


def test_build_follows_the_eval_header():
    """the library is rebuilt when include/ivit_eval.h is newer than it: the header is among the files build() compares"""
    so = iv.build()
    assert os.path.getmtime(so) >= os.path.getmtime(_abi.EVAL_HEADER)
    assert "ivit_score.h" in _lib.SOURCES
    src = open(os.path.join(ROOT, "i-vit_amd", "_lib.py")).read()
    assert re.search(r"newest = max\(.*_abi\.EVAL_HEADER", src)


def test_score_kernel_compiled_for_gfx950():
    co = _device_code_object(iv.build())
    # the register form (ncls <= 1024) and the rescanning form
    assert re.search(rb"_Z\d+logits_score_kernelILb1EE", co) and re.search(rb"_Z\d+logits_score_kernelILb0EE", co)


# ---------------------------------------------------------------- score_reference: the contract in numpy
def test_score_reference_rank_is_the_topk_order_and_nll_is_fp64_cross_entropy():
    from ivit_amd.predict import score_reference, topk_reference
    rng = np.random.default_rng(5)
    acc = rng.integers(-2 ** 31, 2 ** 31, size=(64, 1000), dtype=np.int64).astype(np.int32)
    scale = rng.uniform(1e-6, 1e-3, size=1000).astype(np.float32)
    scale[::7] *= -1
    idx, _ = topk_reference(acc, scale, 16)
    labels = rng.integers(0, 1000, size=64).astype(np.int64)
    labels[::2] = idx[np.arange(0, 64, 2), rng.integers(0, 16, size=32)]          # half of them among the first 16
    rank, nll = score_reference(acc, scale, labels)
    assert rank.dtype == np.int32 and nll.dtype == np.float64 and rank.shape == nll.shape == (64,)
    near = rank < 16
    assert near.sum() >= 32 and (~near).sum() >= 16, "degenerate test data"
    assert np.array_equal(idx[near, rank[near]], labels[near])
    assert not any(l in row for l, row in zip(labels[~near], idx[~near].tolist()))
    assert np.array_equal(rank, full_order_rank(acc, scale, labels))
    v = torch.from_numpy(acc).float() * torch.from_numpy(scale)
    want = torch.nn.functional.cross_entropy(v.double(), torch.from_numpy(labels), reduction="none").numpy()
    np.testing.assert_allclose(nll, want, rtol=1e-12, atol=0)
    # values a model gives (a spread of tens): the sum matters here, not only the maximum
    acc, scale, labels = random_case(64, 1000, 6)
    rank, nll = score_reference(acc, scale, labels)
    v = torch.from_numpy(acc).float() * torch.from_numpy(scale)
    want = torch.nn.functional.cross_entropy(v.double(), torch.from_numpy(labels), reduction="none").numpy()
    np.testing.assert_allclose(nll, want, rtol=1e-12, atol=0)
    assert np.array_equal(rank, full_order_rank(acc, scale, labels)) and nll.min() > 1.0
    # labels as a list, a torch tensor, int32: the same
    for lab in (labels.tolist(), torch.from_numpy(labels), labels.astype(np.int32)):
        r2, n2 = score_reference(acc, scale, lab)
        assert np.array_equal(r2, rank) and np.array_equal(n2, nll)


@pytest.mark.parametrize("name,acc,scale,labels,ranks", rule_batches(), ids=[c[0] for c in rule_batches()])
def test_score_reference_tie_and_zero_rules(name, acc, scale, labels, ranks):
    from ivit_amd.predict import score_reference, topk_reference
    rank, nll = score_reference(acc, scale, labels)
    assert rank.tolist() == ranks.tolist()
    order, _ = topk_reference(acc[:1], scale, len(scale))
    assert order[0, rank].tolist() == labels.tolist()
    assert np.all(np.isfinite(nll)) and np.all(nll >= 0)
    if name == "all equal":
        np.testing.assert_allclose(nll, math.log(9), rtol=1e-15)


def test_score_reference_out_of_range_labels_and_underflow():
    from ivit_amd.predict import score_reference
    acc, scale, labels = random_case(6, 10, 1)
    good_rank, good_nll = score_reference(acc, scale, labels)
    bad = labels.copy()
    bad[[0, 3, 5]] = (-1, 10, 2 ** 40)
    rank, nll = score_reference(acc, scale, bad)
    assert rank[[0, 3, 5]].tolist() == [INT32_MAX] * 3 and np.all(np.isnan(nll[[0, 3, 5]]))
    assert np.array_equal(rank[[1, 2, 4]], good_rank[[1, 2, 4]]) and np.array_equal(nll[[1, 2, 4]], good_nll[[1, 2, 4]])
    # v - max < -745: exp underflows to zero, the nll stays finite
    acc, scale, labels, want = underflow_case()
    rank, nll = score_reference(acc, scale, labels)
    assert rank.tolist() == [1, 2, 3, 0] and np.all(np.isfinite(nll))
    # `want` uses log1p; the contract's log(sum) with sum = 1.0067 carries the rounding of the sum, 2^-52 absolute
    np.testing.assert_allclose(nll, want, rtol=1e-15, atol=2.0 ** -51)
    # one class: the label is first and certain
    rank, nll = score_reference(np.array([[5], [-7]], np.int32), np.array([0.5], np.float32), [0, 0])
    assert rank.tolist() == [0, 0] and nll.tolist() == [0.0, 0.0]


def test_goldens_nll_is_torchs_fp32_cross_entropy():
    """every golden with the reference's head outputs: the fp64 statement is within 1e-5 absolute (ten fp32 ulps at the 8 - 16
    these values have) of what the reference's criterion computes, F.cross_entropy on the fp32 outputs"""
    from ivit_amd.predict import score_reference
    seen = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))):
        g = load_golden(os.path.basename(path))
        if "logits_int" not in g.files or "logits_scale" not in g.files:
            continue
        seen.append(os.path.basename(path))
        acc, scale = g["logits_int"], g["logits_scale"]
        rng = np.random.default_rng(len(seen))
        for _ in range(4):
            labels = rng.integers(0, acc.shape[1], size=acc.shape[0]).astype(np.int64)
            rank, nll = score_reference(acc, scale, labels)
            v = torch.from_numpy(acc).float() * torch.from_numpy(scale)
            want = torch.nn.functional.cross_entropy(v, torch.from_numpy(labels), reduction="none").numpy()
            np.testing.assert_allclose(nll, want.astype(np.float64), rtol=0, atol=1e-5)
            assert np.array_equal(rank, full_order_rank(acc, scale, labels))
    assert {"micro_vit_b2.npz", "micro_swin_b2.npz", "deit_tiny_b1.npz", "swin_tiny_b1.npz"} <= set(seen)


# ---------------------------------------------------------------- evaluate(loss=True), with score = score_reference
class ScoreStub(StubEngine):
    """StubEngine with the second output kind: 'images' are accumulator rows, `score` is the numpy statement"""

    def __init__(self, scale):
        super().__init__(scale)
        self.scored = []

    def score(self, images, labels):
        from ivit_amd.predict import score_reference
        assert isinstance(labels, torch.Tensor) and labels.dtype == torch.int64 and labels.ndim == 1
        self.scored.append(len(images))
        return score_reference(np.asarray(images, dtype=np.int32), self.scale, labels.numpy())


def test_evaluate_with_loss_counts_as_without_and_averages_the_nll():
    from ivit_amd.predict import evaluate, score_reference
    acc, scale, labels, ranks = _eval_case()
    eng = ScoreStub(scale)
    nll = score_reference(acc, scale, labels)[1]
    plain = evaluate(eng, _batches(acc, labels, 3), topk=(1, 5))
    assert set(plain) == {"n", "correct", "acc"} and eng.scored == []          # loss=False: the old path, the old keys
    out = evaluate(eng, _batches(acc, labels, 3), topk=(1, 5), loss=True)
    assert eng.scored == [3, 3, 1] and len(eng.calls) == 3                     # ragged last batch; predict was not called again
    assert set(out) == {"n", "correct", "acc", "loss"}
    assert {k: out[k] for k in plain} == plain == {"n": 7, "correct": {1: 3, 5: 5}, "acc": {1: 300.0 / 7, 5: 500.0 / 7}}
    np.testing.assert_allclose(out["loss"], nll.mean(), rtol=1e-14)
    # labels as a torch tensor, ranks in another order, a transform in front
    out = evaluate(eng, [(a + 1, torch.from_numpy(l)) for a, l in _batches(acc, labels, 4)], topk=(3, 1, 6), transform=lambda a: a - 1, loss=True)
    assert {k: out[k] for k in plain} == {"n": 7, "correct": {3: 5, 1: 3, 6: 7}, "acc": {3: 500.0 / 7, 1: 300.0 / 7, 6: 100.0}}
    np.testing.assert_allclose(out["loss"], nll.mean(), rtol=1e-14)
    # a rank beyond the model's 10 classes needs no clamp: every label's rank is below 16
    out = evaluate(eng, _batches(acc, labels, 7), topk=(1, 16), loss=True)
    assert out["correct"] == {1: 3, 16: 7} and out["acc"][16] == 100.0
    assert out["correct"] == evaluate(eng, _batches(acc, labels, 7), topk=(1, 16))["correct"]
    # a wrong label never counts and makes the loss NaN; no batches at all is n = 0
    out = evaluate(eng, [(acc[:3], np.array([10, -1, int(labels[2])]))], topk=(1, 5), loss=True)
    assert out["n"] == 3 and out["correct"] == {1: int(ranks[2] < 1), 5: int(ranks[2] < 5)} and math.isnan(out["loss"])
    out = evaluate(eng, [], topk=(1,), loss=True)
    assert out["n"] == 0 and out["correct"] == {1: 0} and math.isnan(out["loss"]) and math.isnan(out["acc"][1])
    with pytest.raises(ValueError):
        evaluate(eng, [], topk=(0, 5), loss=True)


def _loss_worker(rank, world, port, q):
    import torch.distributed as dist
    from ivit_amd import dist as ivdist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    acc, scale, labels, _ = _eval_case()
    eng = ScoreStub(scale)
    out = ivdist.evaluate_sharded(eng, acc, labels, 3, rank, world, topk=(1, 5), loss=True)
    q.put((rank, out, eng.scored))
    dist.barrier()
    dist.destroy_process_group()


def test_evaluate_sharded_with_loss_world2_equals_unsharded():
    """two gloo ranks score their shards of 7 images (4 + 3, in batches of 3); the one all_reduce of [n, hits, loss_sum] leaves the
    unsharded counts exactly, and the unsharded loss up to the order of the sum, on both"""
    import torch.multiprocessing as mp
    from ivit_amd.predict import evaluate
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_loss_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    acc, scale, labels, _ = _eval_case()
    whole = evaluate(ScoreStub(scale), _batches(acc, labels, 3), topk=(1, 5), loss=True)
    assert whole["n"] == 7 and whole["correct"] == {1: 3, 5: 5}
    for _, out, _ in res:
        assert {k: out[k] for k in ("n", "correct", "acc")} == {k: whole[k] for k in ("n", "correct", "acc")}
        np.testing.assert_allclose(out["loss"], whole["loss"], rtol=1e-12)
    assert res[0][2] == [3, 1] and res[1][2] == [3]                      # shards (0, 4) and (4, 7)
