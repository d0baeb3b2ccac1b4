"""Predictions without a GPU: the C ABI's five entries are declared, bound and exported, the top-k kernel is in the gfx950 code
object, `topk_reference` states the contract (values and order), `evaluate` counts what it should — ragged batches, a clamped
top-k, two gloo ranks — and the goldens the GPU tests use carry outputs for which the rule is well defined."""
import glob
import os
import re
import socket
import struct
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden
import ivit_amd as iv
from ivit_amd import _lib

ENTRIES = ("ivit_logits_topk", "ivit_vit_predict", "ivit_swin_predict", "ivit_vit_predict_graph_create",
           "ivit_swin_predict_graph_create")


def test_header_declares_predict_entries():
    hdr = open(os.path.join(ROOT, "include", "ivit.h")).read()
    assert re.search(r"int\s+ivit_logits_topk\s*\(\s*ivit_handle\s+h\s*,\s*const\s+int32_t\s*\*\s*logits\s*,\s*const\s+float\s*\*\s*scale\s*,"
                     r"\s*int\s+batch\s*,\s*int\s+num_classes\s*,\s*int\s+k\s*,\s*int32_t\s*\*\s*idx\s*,\s*float\s*\*\s*val\s*\)", hdr)
    tail = (r"const\s+int8_t\s*\*\s*images\s*,\s*int\s+batch\s*,\s*int\s+nslices\s*,\s*void\s*\*\s*workspace\s*,\s*size_t\s+bytes\s*,"
            r"\s*int32_t\s*\*\s*logits\s*,\s*const\s+float\s*\*\s*head_scale\s*,\s*int\s+k\s*,\s*int32_t\s*\*\s*idx\s*,\s*float\s*\*\s*val")
    for kind in ("vit", "swin"):
        assert re.search(rf"int\s+ivit_{kind}_predict\s*\(\s*ivit_{kind}\s+m\s*,\s*{tail}\s*\)", hdr), kind
        assert re.search(rf"int\s+ivit_{kind}_predict_graph_create\s*\(\s*ivit_{kind}\s+m\s*,\s*{tail}\s*,\s*ivit_graph\s*\*\s*out\s*\)", hdr), kind
    assert int(re.search(r"#define IVIT_VERSION (\d+)", hdr).group(1)) == 111       # additions only: the version stays


def test_predict_entries_bound_and_exported():
    iv.build()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert len(_lib.SIGNATURES["ivit_logits_topk"]) == 8
    assert len(_lib.SIGNATURES["ivit_vit_predict"]) == len(_lib.SIGNATURES["ivit_swin_predict"]) == 11
    assert len(_lib.SIGNATURES["ivit_vit_predict_graph_create"]) == len(_lib.SIGNATURES["ivit_swin_predict_graph_create"]) == 12


def _device_code_object(so_path):
    """The gfx950 ELF inside the library's clang offload bundle (.hip_fatbin)."""
    b = open(so_path, "rb").read()
    i = b.find(b"__CLANG_OFFLOAD_BUNDLE__")
    assert i >= 0, "no offload bundle in the library"
    n = struct.unpack_from("<Q", b, i + 24)[0]
    off = i + 32
    for _ in range(n):
        o, sz, t = struct.unpack_from("<QQQ", b, off)
        off += 24
        name = b[off:off + t].decode()
        off += t
        if "gfx950" in name:
            return b[i + o:i + o + sz]
    raise AssertionError("no gfx950 code object")


def test_topk_kernel_compiled_for_gfx950():
    co = _device_code_object(iv.build())
    # the register form (ncls <= 1024) and the rescanning form
    assert re.search(rb"_Z\d+logits_topk_kernelILb1EE", co) and re.search(rb"_Z\d+logits_topk_kernelILb0EE", co)


# ---------------------------------------------------------------- topk_reference: the contract in numpy
def test_topk_reference_values_and_untied_indices_equal_torch():
    from ivit_amd.predict import topk_reference
    rng = np.random.default_rng(5)
    acc = rng.integers(-2 ** 31, 2 ** 31, size=(64, 1000), dtype=np.int64).astype(np.int32)
    scale = rng.uniform(1e-6, 1e-3, size=1000).astype(np.float32)
    scale[::7] *= -1
    idx, val = topk_reference(acc, scale, 16)
    assert idx.dtype == np.int32 and val.dtype == np.float32 and idx.shape == val.shape == (64, 16)
    v = torch.from_numpy(acc).float() * torch.from_numpy(scale)
    tv, ti = torch.topk(v, 16, dim=1)
    assert np.array_equal(val.view(np.uint32), tv.numpy().view(np.uint32))
    untied = np.array([len(np.unique(row)) == row.size for row in v.numpy()])
    assert untied.sum() >= 32, "degenerate test data"
    assert np.array_equal(idx[untied], ti.numpy()[untied].astype(np.int32))
    # small accumulators tie often: values still equal torch's, indices follow the stated rule
    acc = rng.integers(-3, 4, size=(16, 200), dtype=np.int64).astype(np.int32)
    idx, val = topk_reference(acc, np.full(200, 0.5, np.float32), 8)
    tv, _ = torch.topk(torch.from_numpy(acc).float() * 0.5, 8, dim=1)
    assert np.array_equal(val, tv.numpy())
    for b in range(16):
        order = sorted(range(200), key=lambda c: (-float(acc[b, c]), c))[:8]
        assert idx[b].tolist() == order


def test_topk_reference_tie_and_zero_rules():
    from ivit_amd.predict import topk_reference
    # one repeated value: ascending class index
    idx, val = topk_reference(np.full((1, 9), 7, np.int32), np.full(9, 0.25, np.float32), 4)
    assert idx.tolist() == [[0, 1, 2, 3]] and val.tolist() == [[1.75] * 4]
    # equal products from different pairs: 2 * 0.5 == 1 * 1.0 == 4 * 0.25
    acc = np.array([[1, 2, 0, 4, 3]], np.int32)
    scale = np.array([1.0, 0.5, 9.0, 0.25, 0.25], np.float32)
    idx, val = topk_reference(acc, scale, 5)
    assert idx.tolist() == [[0, 1, 3, 4, 2]] and val.tolist() == [[1.0, 1.0, 1.0, 0.75, 0.0]]
    # acc = 0 under a negative scale is -0.0: it ties +0.0, the lower index wins, and val keeps the sign bit
    acc = np.array([[-5, 0, 0, 0, -1]], np.int32)
    scale = np.array([1.0, -1.0, 1.0, -1.0, 1.0], np.float32)
    idx, val = topk_reference(acc, scale, 4)
    assert idx.tolist() == [[1, 2, 3, 4]]
    assert val.view(np.uint32).tolist() == [[0x80000000, 0, 0x80000000, 0xBF800000]]
    # int32 -> float32 is round-to-nearest-even
    acc = np.array([[2 ** 24 + 1, 2 ** 24 + 3, 2 ** 31 - 1, -2 ** 31]], np.int64).astype(np.int32)
    idx, val = topk_reference(acc, np.ones(4, np.float32), 4)
    assert idx.tolist() == [[2, 1, 0, 3]] and val.tolist() == [[2.0 ** 31, 2.0 ** 24 + 4, 2.0 ** 24, -2.0 ** 31]]
    for k in (0, 5, 17):
        with pytest.raises(ValueError):
            topk_reference(acc, np.ones(4, np.float32), k)


# ---------------------------------------------------------------- evaluate: counting, with predict = topk_reference
class StubEngine:
    """an engine whose 'images' are the accumulator rows themselves"""

    def __init__(self, scale):
        self.cfg = SimpleNamespace(num_classes=len(scale))
        self.scale = scale
        self.calls = []

    def predict(self, images, k=5):
        from ivit_amd.predict import topk_reference
        self.calls.append((len(images), k))
        return topk_reference(np.asarray(images, dtype=np.int32), self.scale, k)


def _eval_case(n=7, ncls=10, seed=3):
    """accumulators, scale and labels put at rank 0, 2, 5, 0, 2, 5, ... of each image's order: the counts are known"""
    from ivit_amd.predict import topk_reference
    rng = np.random.default_rng(seed)
    acc = rng.integers(-1000, 1000, size=(n, ncls), dtype=np.int64).astype(np.int32)
    scale = rng.uniform(0.01, 0.02, size=ncls).astype(np.float32)
    order, _ = topk_reference(acc, scale, ncls)
    ranks = np.array([(0, 2, 5)[i % 3] for i in range(n)])
    return acc, scale, order[np.arange(n), ranks].astype(np.int64), ranks


def _batches(acc, labels, size):
    return [(acc[a:a + size], labels[a:a + size]) for a in range(0, len(labels), size)]


def test_evaluate_counts_known_labels_ragged_and_clamped():
    from ivit_amd.predict import evaluate
    acc, scale, labels, ranks = _eval_case()
    eng = StubEngine(scale)
    out = evaluate(eng, _batches(acc, labels, 3), topk=(1, 5))
    assert out["n"] == 7 and out["correct"] == {1: int((ranks < 1).sum()), 5: int((ranks < 5).sum())} == {1: 3, 5: 5}
    assert out["acc"] == {1: 100.0 * 3 / 7, 5: 100.0 * 5 / 7}
    assert eng.calls == [(3, 5), (3, 5), (1, 5)]                       # ragged last batch; k = max(topk)
    # labels as a torch tensor, a rank between, a transform in front
    out = evaluate(eng, [(a + 1, torch.from_numpy(l)) for a, l in _batches(acc, labels, 4)], topk=(3, 1, 6), transform=lambda a: a - 1)
    assert out == {"n": 7, "correct": {3: 5, 1: 3, 6: 7}, "acc": {3: 500.0 / 7, 1: 300.0 / 7, 6: 100.0}}
    # max(topk) beyond the model's classes: clamped to the 10 there are, and every label is among them
    eng.calls.clear()
    out = evaluate(eng, _batches(acc, labels, 7), topk=(1, 16))
    assert eng.calls == [(7, 10)] and out["correct"] == {1: 3, 16: 7} and out["acc"][16] == 100.0
    # a wrong label never counts; no batches at all is n = 0
    assert evaluate(eng, [(acc[:2], np.array([10, -1]))], topk=(1, 5))["correct"] == {1: 0, 5: 0}
    assert evaluate(eng, [], topk=(1,))["n"] == 0
    with pytest.raises(ValueError):
        evaluate(eng, [], topk=(0, 5))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _eval_worker(rank, world, port, q):
    import torch.distributed as dist
    from ivit_amd import dist as ivdist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    acc, scale, labels, _ = _eval_case()
    eng = StubEngine(scale)
    out = ivdist.evaluate_sharded(eng, acc, labels, 3, rank, world, topk=(1, 5))
    q.put((rank, out, eng.calls))
    dist.barrier()
    dist.destroy_process_group()


def test_evaluate_sharded_world2_equals_unsharded():
    """two gloo ranks evaluate their shards of 7 images (4 + 3, in batches of 3); the one all_reduce leaves the unsharded counts on both"""
    import torch.multiprocessing as mp
    from ivit_amd.predict import evaluate
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_eval_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    acc, scale, labels, _ = _eval_case()
    whole = evaluate(StubEngine(scale), _batches(acc, labels, 3), topk=(1, 5))
    assert whole == {"n": 7, "correct": {1: 3, 5: 5}, "acc": {1: 300.0 / 7, 5: 500.0 / 7}}
    assert res[0][1] == whole and res[1][1] == whole
    assert res[0][2] == [(3, 5), (1, 5)] and res[1][2] == [(3, 5)]     # shards (0, 4) and (4, 7)


# ---------------------------------------------------------------- the fixtures the GPU tests compare against
def test_goldens_with_logits_have_a_well_defined_topk():
    """every golden that records the reference's head outputs (logits_int, logits_scale): the scale is finite (the contract's one
    precondition), the rule gives k distinct classes in non-increasing value order, and the values are the recorded products"""
    from ivit_amd.predict import MAX_K, topk_reference
    seen = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))):
        g = load_golden(os.path.basename(path))
        if "logits_int" not in g.files or "logits_scale" not in g.files:
            continue
        seen.append(os.path.basename(path))
        acc, scale = g["logits_int"], g["logits_scale"]
        assert acc.dtype == np.int32 and acc.ndim == 2 and scale.dtype == np.float32 and scale.shape == (acc.shape[1],)
        assert np.all(np.isfinite(scale))
        k = min(MAX_K, acc.shape[1])
        idx, val = topk_reference(acc, scale, k)
        assert np.all(np.isfinite(val)) and np.all(np.diff(val, axis=1) <= 0)
        assert all(len(set(row)) == k for row in idx.tolist()) and idx.min() >= 0 and idx.max() < acc.shape[1]
        assert np.array_equal(val, (acc.astype(np.float32) * scale)[np.arange(len(acc))[:, None], idx])
    assert {"micro_vit_b2.npz", "micro_swin_b2.npz", "deit_tiny_b1.npz", "swin_tiny_b1.npz"} <= set(seen)
