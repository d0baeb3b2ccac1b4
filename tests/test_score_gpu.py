"""The score on the device.  Operator: ivit_logits_score against `score_reference` — rank exactly, nll within atol 1e-9 / rtol 1e-12
(the derived bound is (num_classes + 16) * 2^-53 * max(1, |nll|), 1.1e-13 at 1000 classes) — over the shapes at which the kernel
changes path (one class, under / at / over one class per lane, the last register slot, the register form's limit of 1024, the
rescanning form with a ragged tail; a block with missing wavefronts) and over contents that make the order matter; its arguments and
its memory contract.  Models: score / capture_score of both engines against the numpy statement and against predict, and
evaluate(loss=True), which must count what evaluate counts without synchronising."""
import numpy as np
import pytest

from score_cases import INT32_MAX, random_case, rule_batches, underflow_case

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from ivit_amd.predict import evaluate, score_reference  # noqa: E402
from test_predict_gpu import H, P, _engine, dev  # noqa: E402,F401  (H: the module's handle fixture)

GUARD_BYTES = 4096
FILL = 0x5A


def guarded(nbytes):
    """(whole buffer, payload view): `nbytes` of payload between two 4 KiB guards, everything filled with 0x5A"""
    whole = torch.full((GUARD_BYTES + nbytes + GUARD_BYTES,), FILL, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD_BYTES:GUARD_BYTES + nbytes]


def guards_intact(whole, nbytes):
    w = whole.cpu().numpy()
    return bool(np.all(w[:GUARD_BYTES] == FILL) and np.all(w[GUARD_BYTES + nbytes:] == FILL))


def run_score(H, acc, scale, labels, want_rank=True, want_nll=True):
    """ivit_logits_score on host arrays -> (rank or None, nll or None); the guards around both outputs must stay untouched"""
    B, ncls = acc.shape
    d_acc, d_scale, d_lab = dev(acc), dev(scale), dev(np.asarray(labels, dtype=np.int64))     # named: alive until the results are back
    rk_all, rk = guarded(4 * B)
    nl_all, nl = guarded(8 * B)
    H.call("ivit_logits_score", P(d_acc), P(d_scale), P(d_lab), B, ncls, P(rk) if want_rank else None, P(nl) if want_nll else None)
    assert guards_intact(rk_all, 4 * B) and guards_intact(nl_all, 8 * B), "wrote outside its outputs"
    rank, nll = rk.cpu().numpy().view(np.int32), nl.cpu().numpy().view(np.float64)
    if not want_rank:
        assert np.all(rk.cpu().numpy() == FILL)
    if not want_nll:
        assert np.all(nl.cpu().numpy() == FILL)
    return rank if want_rank else None, nll if want_nll else None


def assert_nll(got, want):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=1e-12, atol=1e-9)


def check(H, acc, scale, labels):
    want_rank, want_nll = score_reference(acc, scale, labels)
    rank, nll = run_score(H, acc, scale, labels)
    assert np.array_equal(rank, want_rank), f"ranks differ at images {np.nonzero(rank != want_rank)[0][:4]}"
    assert_nll(nll, want_nll)


NCLS = [1, 10, 63, 64, 65, 1000, 1024, 1025, 4099]
BATCHES = [1, 4, 5, 7]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("ncls", NCLS)
def test_score_random(H, ncls, B):
    """values spread over a few tens (every class weighs in the sum), then uniform int32 accumulators (the maximum alone decides);
    random labels, then labels at class 0 and num_classes - 1"""
    acc, scale, labels = random_case(B, ncls, 1000 * ncls + B)
    check(H, acc, scale, labels)
    check(H, acc, scale, np.where(np.arange(B) % 2 == 0, 0, ncls - 1))
    rng = np.random.default_rng(ncls * 7 + B)
    acc = rng.integers(-2 ** 31, 2 ** 31, size=(B, ncls), dtype=np.int64).astype(np.int32)
    scale = rng.uniform(1e-6, 1e-3, size=ncls).astype(np.float32)
    scale[::7] *= -1
    check(H, acc, scale, labels)


@pytest.mark.parametrize("name,acc,scale,labels,ranks", rule_batches(), ids=[c[0] for c in rule_batches()])
def test_score_tie_and_zero_rules(H, name, acc, scale, labels, ranks):
    rank, nll = run_score(H, acc, scale, labels)
    assert rank.tolist() == ranks.tolist()
    assert_nll(nll, score_reference(acc, scale, labels)[1])


@pytest.mark.parametrize("ncls", [65, 1000, 1025, 4099])
def test_score_ties_across_lanes_and_register_slots(H, ncls):
    """one repeated value, then zeros of both signs, over a whole row: every class ties, so rank == label — at the first and last
    lane, the first class of the second register slot, the last class, and (rescanning form) classes beyond 1024"""
    labels = np.array(sorted({0, 1, 63, 64, ncls // 2, min(1024, ncls - 1), ncls - 2, ncls - 1}), np.int64)
    B = len(labels)
    scale = np.where(np.arange(ncls) % 3 == 0, -0.5, 0.5).astype(np.float32)
    for acc in (np.tile(np.where(scale < 0, -14, 14).astype(np.int32), (B, 1)), np.zeros((B, ncls), np.int32)):
        rank, nll = run_score(H, acc, scale, labels)
        assert rank.tolist() == labels.tolist()
        np.testing.assert_allclose(nll, np.log(float(ncls)), rtol=1e-12, atol=1e-9)
        check(H, acc, scale, labels)


@pytest.mark.parametrize("ncls", [10, 1025])
def test_score_out_of_range_labels(H, ncls):
    """-1, num_classes and labels whose low 32 bits would be a valid class: rank INT32_MAX, nll NaN, the neighbours unharmed"""
    acc, scale, labels = random_case(9, ncls, 77 + ncls)
    bad = labels.copy()
    bad[[0, 2, 4, 5, 8]] = (-1, ncls, 2 ** 32 + 3, -2 ** 63, 2 ** 63 - 1)
    rank, nll = run_score(H, acc, scale, bad)
    want_rank, want_nll = score_reference(acc, scale, bad)
    assert rank[[0, 2, 4, 5, 8]].tolist() == [INT32_MAX] * 5 and np.all(np.isnan(nll[[0, 2, 4, 5, 8]]))
    assert np.array_equal(rank, want_rank)
    assert_nll(nll, want_nll)
    assert np.all(np.isfinite(nll[[1, 3, 6, 7]]))


def test_score_underflowing_spread(H):
    acc, scale, labels, want = underflow_case()
    rank, nll = run_score(H, acc, scale, labels)
    assert rank.tolist() == [1, 2, 3, 0] and np.all(np.isfinite(nll))
    np.testing.assert_allclose(nll, want, rtol=1e-12, atol=1e-9)
    assert_nll(nll, score_reference(acc, scale, labels)[1])


def test_score_arguments(H):
    acc, scale, labels = random_case(6, 100, 9)
    want_rank, want_nll = score_reference(acc, scale, labels)
    rank, none = run_score(H, acc, scale, labels, want_nll=False)                 # nll = NULL: ranks only
    assert none is None and np.array_equal(rank, want_rank)
    none, nll = run_score(H, acc, scale, labels, want_rank=False)                 # rank = NULL: losses only
    assert none is None
    assert_nll(nll, want_nll)
    # refused with IVIT_ERR_INVALID and nothing launched (the outputs keep their fill): both outputs NULL, a missing input,
    # a negative batch, no classes
    d_acc, d_scale, d_lab = dev(acc), dev(scale), dev(labels)
    rk = torch.full((6,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    nl = torch.full((6,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    f = H.lib.ivit_logits_score
    for args in ((P(d_acc), P(d_scale), P(d_lab), 6, 100, None, None),
                 (None, P(d_scale), P(d_lab), 6, 100, P(rk), P(nl)),
                 (P(d_acc), None, P(d_lab), 6, 100, P(rk), P(nl)),
                 (P(d_acc), P(d_scale), None, 6, 100, P(rk), P(nl)),
                 (P(d_acc), P(d_scale), P(d_lab), -1, 100, P(rk), P(nl)),
                 (P(d_acc), P(d_scale), P(d_lab), 6, 0, P(rk), P(nl)),
                 (P(d_acc), P(d_scale), P(d_lab), 6, -5, P(rk), P(nl))):
        assert f(H.h, *args) == _lib.IVIT_ERR_INVALID, args[3:5]
    assert f(None, P(d_acc), P(d_scale), P(d_lab), 6, 100, P(rk), P(nl)) == _lib.IVIT_ERR_INVALID
    assert f(H.h, P(d_acc), P(d_scale), P(d_lab), 0, 100, P(rk), P(nl)) == _lib.IVIT_OK           # empty batch
    torch.cuda.synchronize()
    assert bool((rk == 0x5A5A5A5A).all()) and bool((nl == 0x5A5A5A5A5A5A5A5A).all())


@pytest.mark.parametrize("ncls", [1000, 1025])
def test_score_memory_contract_and_odd_offset(H, ncls):
    """logits, scale and labels keep their bytes (and the bytes around them); logits may start at any int32, here an odd one"""
    B = 5
    acc, scale, labels = random_case(B, ncls, 5 + ncls)
    ins = {}
    for name, a, lead in (("logits", acc, 4), ("scale", scale, 0), ("labels", labels, 0)):
        whole, view = guarded(lead + a.nbytes)                                 # lead = 4: the payload starts at an odd int32
        view[lead:].copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)))
        ins[name] = (whole, view[lead:], whole.clone())
    assert ins["logits"][1].data_ptr() % 8 == 4
    rk_all, rk = guarded(4 * B)
    nl_all, nl = guarded(8 * B)
    H.call("ivit_logits_score", P(ins["logits"][1]), P(ins["scale"][1]), P(ins["labels"][1]), B, ncls, P(rk), P(nl))
    torch.cuda.synchronize()
    for name, (whole, _, before) in ins.items():
        assert torch.equal(whole, before), f"{name} or its surroundings changed"
    assert guards_intact(rk_all, 4 * B) and guards_intact(nl_all, 8 * B)
    want_rank, want_nll = score_reference(acc, scale, labels)
    assert np.array_equal(rk.cpu().numpy().view(np.int32), want_rank)
    assert_nll(nl.cpu().numpy().view(np.float64), want_nll)


# ---------------------------------------------------------------- models
MODELS = ["micro_vit_b2.npz", "micro_swin_b2.npz"]


@pytest.fixture(scope="module", params=MODELS)
def model(request):
    return _engine(request.param)


def _labels_at(eng, imgs, ranks):
    """labels = the class each image's own prediction puts at ranks[i]"""
    order = eng.predict(imgs, k=int(max(ranks)) + 1, copy=True)[0].cpu().numpy()
    return torch.from_numpy(order[np.arange(len(ranks)), ranks].astype(np.int64)).cuda()


def test_engine_score_equals_reference_and_agrees_with_predict(model):
    g, cfg, eng = model
    B = 7
    imgs = dev(iv.make_images_int8(cfg, B, seed=41))
    k = min(6, cfg.num_classes)
    idx = eng.predict(imgs, k=k, copy=True)[0].cpu().numpy()
    logits = eng.last_logits.cpu().numpy()
    scale = eng.head_scale_host()
    labels = np.random.default_rng(3).integers(0, cfg.num_classes, size=B).astype(np.int64)
    labels[:3] = idx[np.arange(3), [0, 2, k - 1]]                                # three of them among the first k for certain
    d_labels = dev(labels)
    want_rank, want_nll = score_reference(logits, scale, labels)
    for nslices in (1, 2):
        eng.forward(imgs, nslices=nslices).zero_()                               # score must write the logits buffer itself
        rank, nll = eng.score(imgs, d_labels, nslices=nslices)
        assert rank.dtype == torch.int32 and nll.dtype == torch.float64 and rank.shape == nll.shape == (B,)
        assert np.array_equal(eng.last_logits.cpu().numpy(), logits), nslices
        assert np.array_equal(rank.cpu().numpy(), want_rank), nslices
        assert_nll(nll.cpu().numpy(), want_nll)
    rank = rank.cpu().numpy()
    assert rank[:3].tolist() == [0, 2, k - 1]
    for j in range(1, k + 1):                                                    # rank < j  <=>  the label is among the first j
        assert np.array_equal(rank < j, (idx[:, :j] == labels[:, None]).any(axis=1)), j
    a = eng.score(imgs, d_labels)
    b = eng.score(imgs, d_labels, copy=True)
    assert a[0].data_ptr() == eng.score(imgs, d_labels)[0].data_ptr() != b[0].data_ptr() and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for wrong in (d_labels.cpu(), d_labels.to(torch.int32), d_labels[:B - 1], d_labels.reshape(B, 1)):
        with pytest.raises(AssertionError):
            eng.score(imgs, wrong)
    st = getattr(eng.h.lib, eng.PREFIX + "_score")(*eng._score_args(imgs, d_labels, 1)[0][:-2], None, None)
    assert st == _lib.IVIT_ERR_INVALID                                           # both outputs NULL: refused before the forward


def test_capture_score_replays_on_changed_images_and_labels(model):
    """one hipGraph of forward + score, replayed on changing image AND label contents: the graph reads both buffers again"""
    g, cfg, eng = model
    B = 3
    buf = dev(iv.make_images_int8(cfg, B, seed=1))
    lab = torch.zeros(B, dtype=torch.int64, device="cuda")
    replay = eng.capture_score(buf, lab, nstreams=2)
    for seed in (21, 22, 23):
        imgs = dev(iv.make_images_int8(cfg, B, seed=seed))
        labels = dev(np.random.default_rng(seed).integers(0, cfg.num_classes, size=B).astype(np.int64))
        want_rank, want_nll = eng.score(imgs, labels, nslices=1, copy=True)
        want_logits = eng.last_logits.clone()
        buf.copy_(imgs)
        lab.copy_(labels)
        rank, nll = replay()
        torch.cuda.synchronize()
        assert torch.equal(rank, want_rank) and torch.equal(nll, want_nll), seed
        assert torch.equal(eng._native_buffers(B, 2)[1], want_logits)
        ref_rank, ref_nll = score_reference(want_logits.cpu().numpy(), eng.head_scale_host(), labels.cpu().numpy())
        assert np.array_equal(rank.cpu().numpy(), ref_rank)
        assert_nll(nll.cpu().numpy(), ref_nll)
    lab.fill_(-1)                                                                # the label buffer alone changes
    rank, nll = replay()
    torch.cuda.synchronize()
    assert rank.tolist() == [INT32_MAX] * B and bool(torch.isnan(nll).all())


def test_evaluate_with_loss_on_models(model):
    """7 images in batches of 3 (ragged): the counts of evaluate(loss=False), the loss of the numpy statement; a top-16 on a
    10-class model; a bad label"""
    g, cfg, eng = model
    imgs = dev(iv.make_images_int8(cfg, 7, seed=31))
    labels = _labels_at(eng, imgs, np.array([(0, 2, 5)[i % 3] for i in range(7)]))
    batches = lambda lab: [(imgs[a:a + 3], lab[a:a + 3]) for a in range(0, 7, 3)]      # noqa: E731
    plain = evaluate(eng, batches(labels), topk=(1, 5))
    assert plain == {"n": 7, "correct": {1: 3, 5: 5}, "acc": {1: 300.0 / 7, 5: 500.0 / 7}}
    out = evaluate(eng, batches(labels), topk=(1, 5), loss=True)
    assert set(out) == {"n", "correct", "acc", "loss"} and {k: out[k] for k in plain} == plain
    logits = eng.forward(imgs).cpu().numpy()
    want = score_reference(logits, eng.head_scale_host(), labels.cpu().numpy())[1]
    np.testing.assert_allclose(out["loss"], want.mean(), rtol=1e-12, atol=1e-9)
    out = evaluate(eng, batches(labels.cpu()), topk=(1, 16), loss=True)               # host labels; beyond TOPK_MAX_K is no matter
    assert out["correct"] == {1: 3, 16: 7}
    np.testing.assert_allclose(out["loss"], want.mean(), rtol=1e-12, atol=1e-9)
    bad = labels.clone()
    bad[4] = cfg.num_classes
    out = evaluate(eng, batches(bad), topk=(1, 5), loss=True)
    assert out["n"] == 7 and out["correct"] == {1: 3, 5: 4} and np.isnan(out["loss"])  # image 4 was a top-3 hit


def test_evaluate_with_loss_does_not_synchronise(model):
    """pattern of test_evaluate_loop_does_not_synchronise: with device labels, torch raises on any synchronising call while the
    batches are being consumed; the read of [n, hits, loss_sum] comes after"""
    from ivit_amd import dist as ivdist
    from ivit_amd import preprocess as pp
    g, cfg, eng = model
    S = cfg.img_size                                                        # pixels [7, S + 8, S + 12, 3] -> resize S + 4 -> crop S
    u8 = dev(np.random.default_rng(4).integers(0, 256, size=(7, S + 8, S + 12, 3), dtype=np.uint8))
    s_in = np.float32(g["scale/qact_input"])
    tf = lambda x: pp.eval_transform(x, s_in, S + 4, S)      # noqa: E731
    d_labels = _labels_at(eng, tf(u8), np.array([(0, 2, 5)[i % 3] for i in range(7)]))
    want = evaluate(eng, [(u8[:3], d_labels[:3]), (u8[6:], d_labels[6:])], transform=tf, loss=True)      # buffers of both batch shapes exist
    assert want["n"] == 4

    def watched(batches):
        torch.cuda.set_sync_debug_mode("error")
        try:
            yield from batches
        finally:
            torch.cuda.set_sync_debug_mode("default")

    try:                                                                    # whatever fails, the mode does not outlive the test
        out = evaluate(eng, watched([(u8[a:a + 3], d_labels[a:a + 3]) for a in range(0, 7, 3)]), topk=(1, 5), transform=tf, loss=True)
        assert torch.cuda.get_sync_debug_mode() == 0
        assert out["n"] == 7 and out["correct"] == {1: 3, 5: 5} and np.isfinite(out["loss"])
        # the watch is live on this runtime: a device-to-host read under it raises
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):
                d_labels.cpu()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        sharded = ivdist.evaluate_sharded(eng, u8, d_labels.cpu(), 3, 0, 1, transform=tf, loss=True)
        assert sharded == out
    finally:
        torch.cuda.set_sync_debug_mode("default")
