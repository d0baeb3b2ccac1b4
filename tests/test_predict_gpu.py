"""Predictions on the device.  Operator: ivit_logits_topk against `topk_reference` — indices exactly, values as bit patterns — over the
shapes at which the kernel changes path (one class, under / at / over one class per lane, the register form's limit of 1024, the
rescanning form beyond it, a block with missing wavefronts) and over contents that make the order matter.  Models: predict /
capture_predict of both engines against the reference's recorded head outputs, and evaluate's counts, single and over two ranks."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden, golden_scales

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from ivit_amd.predict import evaluate, topk_reference  # noqa: E402

_P = ctypes.c_void_p
GUARD = 0x5A5A5A5A


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


def P(t):
    return _P(t.data_ptr())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_topk(H, acc, scale, k, with_val=True):
    """ivit_logits_topk on host arrays -> (idx, val bits or None); one guard row behind each output must stay untouched"""
    B, ncls = acc.shape
    idx = torch.full((B + 1, k), GUARD, dtype=torch.int32, device="cuda")
    val = torch.full((B + 1, k), GUARD, dtype=torch.int32, device="cuda")            # float bits, kept as integers
    d_acc, d_scale = dev(acc), dev(scale)                                             # named: alive until the results are back
    H.call("ivit_logits_topk", P(d_acc), P(d_scale), B, ncls, k, P(idx), P(val) if with_val else None)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    assert np.all(idx[B] == GUARD) and np.all(val[B] == GUARD), "wrote behind its outputs"
    if not with_val:
        assert np.all(val == GUARD)
    return idx[:B], val[:B].view(np.uint32) if with_val else None


def check(H, acc, scale, k):
    ri, rv = topk_reference(acc, scale, k)
    gi, gv = run_topk(H, acc, scale, k)
    assert np.array_equal(gi, ri), f"{(gi != ri).sum()} indices differ; first rows {np.nonzero((gi != ri).any(1))[0][:4]}"
    assert np.array_equal(gv, rv.view(np.uint32))


SHAPES = [(1, 1, 1), (1, 10, 1), (3, 10, 10), (5, 63, 5), (4, 64, 16), (5, 65, 5), (7, 1000, 5), (2, 1000, 16), (3, 1001, 8),
          (2, 1024, 16), (2, 1025, 5), (2, 4100, 16), (301, 1000, 5)]


@pytest.mark.parametrize("B,ncls,k", SHAPES)
def test_topk_uniform_random(H, B, ncls, k):
    """uniform int32 accumulators, scales of both signs.  (2, 4100, 16) is the rescanning form; (301, 1000, 5) is 76 blocks of four
    wavefronts, the last with one image."""
    rng = np.random.default_rng(B * 100003 + ncls * 17 + k)
    acc = rng.integers(-2 ** 31, 2 ** 31, size=(B, ncls), dtype=np.int64).astype(np.int32)
    scale = rng.uniform(1e-6, 1e-3, size=ncls).astype(np.float32)
    scale[rng.random(ncls) < 0.3] *= -1
    check(H, acc, scale, k)


@pytest.mark.parametrize("B,ncls,k", SHAPES)
def test_topk_ordered_contents(H, B, ncls, k):
    """contents where the order is the whole answer, at every shape: image by image in turn
      0  one repeated value;
      1  over half the classes tied at the maximum, the rest below;
      2  equal products from different pairs (acc 2 * scale 0.5 beside acc 1 * scale 1.0) among small values;
      3  acc = 0 everywhere, scales of both signs: -0.0 ties +0.0, the lower index wins, val keeps the sign;
      4  the int32 -> fp32 rounding cases +-(2^31 - 1), -2^31, 2^24 + 1 (and 2^24, 2^24 + 2 they must tie with or fall between);
      5  the top k all in ONE lane's classes (c = 5 mod 64) where the shape has them, else in the first k classes;
      6  the top k in the last partial group of 64 classes, descending towards the end."""
    rng = np.random.default_rng(ncls * 31 + k)
    B7 = max(B, 7) if B < 100 else B
    scale = np.ones(ncls, np.float32)
    scale[1::2] = 0.5                                                       # exact powers of two: products tie exactly
    neg = rng.random(ncls) < 0.4
    acc = np.zeros((B7, ncls), np.int64)
    for b in range(B7):
        kind = b % 7
        if kind == 0:
            acc[b] = 12 * np.where(scale == 0.5, 2, 1)                      # every product 12.0
        elif kind == 1:
            tied = rng.random(ncls) < 0.6
            acc[b] = np.where(tied, 1000, rng.integers(-1000, 1000, ncls)) * np.where(scale == 0.5, 2, 1)
        elif kind == 2:
            acc[b] = rng.integers(-3, 4, ncls) * np.where(scale == 0.5, 2, 1) + (rng.random(ncls) < 0.2)
        elif kind == 3:
            acc[b] = 0
        elif kind == 4:
            acc[b] = rng.choice([2 ** 31 - 1, -(2 ** 31 - 1), -2 ** 31, 2 ** 24 + 1, 2 ** 24, 2 ** 24 + 2, 2 ** 31 - 64, 2 ** 31 - 65], ncls)
        elif kind == 5:
            acc[b] = rng.integers(-1000, 1000, ncls)
            lane = np.arange(5, ncls, 64)
            own = lane if len(lane) >= k else np.arange(k)
            acc[b, own] = 10 ** 6 + 4 * rng.permutation(len(own))
        else:
            acc[b] = rng.integers(-1000, 1000, ncls)
            first = (ncls - 1) // 64 * 64
            tail = np.arange(first, ncls) if ncls - first >= k else np.arange(ncls - k, ncls)
            acc[b, tail] = 10 ** 6 + 4 * np.arange(len(tail))
    acc = acc.astype(np.int32)
    for s in (scale, np.where(neg, -scale, scale).astype(np.float32)):
        check(H, acc, s, k)
    if ncls >= 4:                                                           # the zero rule is in play, and lower indices do win
        i3, v3 = topk_reference(acc[3:4], np.where(neg, -scale, scale).astype(np.float32), min(k, 4))
        assert i3[0].tolist() == list(range(min(k, 4))) and set(v3.view(np.uint32).ravel().tolist()) <= {0, 0x80000000}


def test_topk_arguments(H):
    rng = np.random.default_rng(9)
    acc = rng.integers(-10 ** 6, 10 ** 6, size=(6, 100), dtype=np.int64).astype(np.int32)
    scale = rng.uniform(0.5, 1.5, size=100).astype(np.float32)
    gi, gv = run_topk(H, acc, scale, 5, with_val=False)                    # val = NULL: indices only
    assert gv is None and np.array_equal(gi, topk_reference(acc, scale, 5)[0])
    # k outside 1 .. min(16, ncls): IVIT_ERR_INVALID and nothing launched (the outputs keep their fill)
    idx = torch.full((6, 17), GUARD, dtype=torch.int32, device="cuda")
    val = torch.full((6, 17), GUARD, dtype=torch.int32, device="cuda")
    d_acc, d_scale = dev(acc), dev(scale)
    for ncls, k in ((100, 0), (100, 17), (100, -1), (10, 11), (1, 2)):
        st = H.lib.ivit_logits_topk(H.h, P(d_acc), P(d_scale), 6, ncls, k, P(idx), P(val))
        assert st == _lib.IVIT_ERR_INVALID, (ncls, k, st)
    st = H.lib.ivit_logits_topk(H.h, P(d_acc), P(d_scale), 6, 100, 5, None, P(val))
    assert st == _lib.IVIT_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((idx == GUARD).all()) and bool((val == GUARD).all())
    assert H.lib.ivit_logits_topk(H.h, P(d_acc), P(d_scale), 0, 100, 5, P(idx), P(val)) == _lib.IVIT_OK     # empty batch


# ---------------------------------------------------------------- models
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
    return g, cfg, eng


@pytest.fixture(scope="module")
def micro_vit():
    return _engine("micro_vit_b2.npz")


@pytest.mark.parametrize("fname", ["micro_vit_b2.npz", "micro_swin_b2.npz", "deit_tiny_b1.npz", "swin_tiny_b1.npz"])
def test_predict_equals_reference_rule_on_golden_outputs(fname):
    """predict(k) == topk_reference of the REFERENCE's recorded accumulators and head scale; the logits it leaves are forward's;
    two slices give the same; both spellings of the head scale's host copy agree with the recorded one"""
    g, cfg, eng = _engine(fname)
    imgs = dev(iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"])))
    assert np.array_equal(eng.head_scale_host(), g["logits_scale"])
    old = eng.head_scale() if callable(eng.head_scale) else eng.head_scale
    assert np.array_equal(old, g["logits_scale"])
    fwd = eng.forward(imgs).cpu().numpy()
    assert np.array_equal(fwd, g["logits_int"])
    for k in (1, 5, min(16, cfg.num_classes)):
        ri, rv = topk_reference(g["logits_int"], g["logits_scale"], k)
        for nslices in (1, 2):
            eng.forward(imgs).zero_()                                       # predict must write the logits buffer itself
            idx, val = eng.predict(imgs, k=k, nslices=nslices)
            assert idx.dtype == torch.int32 and val.dtype == torch.float32 and idx.shape == val.shape == (imgs.shape[0], k)
            assert np.array_equal(idx.cpu().numpy(), ri), (k, nslices)
            assert np.array_equal(val.cpu().numpy().view(np.uint32), rv.view(np.uint32)), (k, nslices)
            assert np.array_equal(eng.last_logits.cpu().numpy(), g["logits_int"])
    a = eng.predict(imgs, k=5)
    b = eng.predict(imgs, k=5, copy=True)
    assert a[0].data_ptr() == eng.predict(imgs, k=5)[0].data_ptr() != b[0].data_ptr() and torch.equal(a[0], b[0])
    with pytest.raises(_lib.IvitError):
        eng.predict(imgs, k=17)
    with pytest.raises(_lib.IvitError):
        eng.predict(imgs, k=0)


@pytest.mark.parametrize("fname", ["micro_vit_b2.npz", "micro_swin_b2.npz"])
def test_capture_predict_replays_equal_predict(fname):
    """one hipGraph of forward + top-k, replayed three times on changing image contents (the graph reads the caller's image buffer)"""
    g, cfg, eng = _engine(fname)
    B = 3
    buf = dev(iv.make_images_int8(cfg, B, seed=1))
    replay = eng.capture_predict(buf, k=5, nstreams=2)
    for seed in (21, 22, 23):
        imgs = dev(iv.make_images_int8(cfg, B, seed=seed))
        want_idx, want_val = eng.predict(imgs, k=5, nslices=1, copy=True)
        want_logits = eng.last_logits.clone()
        buf.copy_(imgs)
        idx, val = replay()
        torch.cuda.synchronize()
        assert torch.equal(idx, want_idx) and torch.equal(val.view(torch.int32), want_val.view(torch.int32)), seed
        assert torch.equal(eng._native_buffers(B, 2)[1], want_logits)


def _labelled(eng, imgs, n):
    """labels = the class each image's own prediction ranks 1st, 3rd, 6th by turns -> (labels, {1: hits, 5: hits})"""
    order = eng.predict(imgs, k=6, copy=True)[0].cpu().numpy()
    ranks = np.array([(0, 2, 5)[i % 3] for i in range(n)])
    return torch.from_numpy(order[np.arange(n), ranks].astype(np.int64)), {1: int((ranks < 1).sum()), 5: int((ranks < 5).sum())}


def test_evaluate_counts_on_micro_vit(micro_vit):
    """7 images in batches of 3 (ragged); the same through eval_transform from uint8 pixels; a top-k beyond the 10 classes"""
    from ivit_amd import preprocess as pp
    g, cfg, eng = micro_vit
    imgs = dev(iv.make_images_int8(cfg, 7, seed=31))
    labels, expect = _labelled(eng, imgs, 7)
    assert expect == {1: 3, 5: 5}
    out = evaluate(eng, [(imgs[a:a + 3], labels[a:a + 3]) for a in range(0, 7, 3)], topk=(1, 5))
    assert out == {"n": 7, "correct": expect, "acc": {1: 300.0 / 7, 5: 500.0 / 7}}
    out = evaluate(eng, [(imgs[a:a + 3], labels[a:a + 3].cuda()) for a in range(0, 7, 3)], topk=(1, 16))
    assert out["correct"] == {1: 3, 16: 7}
    # uint8 pixels [7, 40, 44, 3] -> resize 36 -> crop 32 -> normalise -> input QuantAct, inside evaluate
    u8 = dev(np.random.default_rng(4).integers(0, 256, size=(7, 40, 44, 3), dtype=np.uint8))
    tf = lambda x: pp.eval_transform(x, eng.f32["s_in"], 36, cfg.img_size)      # noqa: E731
    labels, expect = _labelled(eng, tf(u8), 7)
    out = evaluate(eng, [(u8[a:a + 3], labels[a:a + 3]) for a in range(0, 7, 3)], topk=(1, 5), transform=tf)
    assert out["n"] == 7 and out["correct"] == expect == {1: 3, 5: 5}


def test_evaluate_loop_does_not_synchronise(micro_vit, monkeypatch):
    """with labels on the device, nothing between the first batch and the last synchronises the host with the GPU or copies between
    them: torch raises on any such call while the batches are being consumed (the final read of the counts comes after)"""
    from ivit_amd import dist as ivdist
    from ivit_amd import preprocess as pp
    g, cfg, eng = micro_vit
    u8 = dev(np.random.default_rng(4).integers(0, 256, size=(7, 40, 44, 3), dtype=np.uint8))
    tf = lambda x: pp.eval_transform(x, eng.f32["s_in"], 36, cfg.img_size)      # noqa: E731
    labels, expect = _labelled(eng, tf(u8), 7)
    d_labels = labels.cuda()
    evaluate(eng, [(u8[:3], d_labels[:3]), (u8[6:], d_labels[6:])], transform=tf)          # buffers of both batch shapes exist

    def watched(batches):
        torch.cuda.set_sync_debug_mode("error")
        try:
            yield from batches
        finally:
            torch.cuda.set_sync_debug_mode("default")

    try:                                                                    # whatever fails, the mode does not outlive the test
        out = evaluate(eng, watched([(u8[a:a + 3], d_labels[a:a + 3]) for a in range(0, 7, 3)]), topk=(1, 5), transform=tf)
        assert torch.cuda.get_sync_debug_mode() == 0
        assert out["n"] == 7 and out["correct"] == expect
        # the watch is live on this runtime: a device-to-host read under it raises
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):
                d_labels.cpu()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        # evaluate_sharded uploads a rank's host labels once, before the loop: its loop passes the same watch
        import ivit_amd.predict as pred
        monkeypatch.setattr(pred, "evaluate", lambda e, b, **kw: evaluate(e, watched(b), **kw))
        out = ivdist.evaluate_sharded(eng, u8, labels, 3, 0, 1, transform=tf)
        assert torch.cuda.get_sync_debug_mode() == 0
        assert out["n"] == 7 and out["correct"] == expect
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_evaluate_sharded_over_two_ranks():
    """tools/dist_eval_check.py as two ranks on one GPU over gloo (a fresh child process under its own time limit): the counts after the
    one all_reduce equal the single-process ones and the known ones"""
    import os
    import socket
    import subprocess
    import sys
    from conftest import ROOT
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, IVIT_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), "tools/dist_eval_check.py", "micro_vit2h_b3.npz", "7"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "EVAL_CHECK_OK world 2 n 7 correct {1: 3, 5: 5} expected {1: 3, 5: 5} shards [(0, 4), (4, 7)]" in r.stdout
