"""Linear probe on the device (include/ivit_probe.h).  Everything is bit-exact against `predict.probe_stats_reference`: array_equal
on the three int64 arrays — the WHOLE Gram matrix, so its symmetry is covered — no tolerance anywhere.

The sweep crosses widths (one column block, one and a half, three, eight), row counts (one row, a partial k-step, one row over a
k-step, several 64-row chunks and one row over), class counts (both forms of the class sums: privatised in LDS, straight global adds)
and the number of parts (0 = the library's choice, 1, 3); full-range int8 including -128; two calls into the same buffers give the
sum, every array between guard bands.  Then the int32 bound (131 073 rows of -128: every Gram entry above 2^31), the ignore labels
(-1, num_classes, 2^32 + 3, 2^40), the empty call and the refusals (outputs untouched), a hipGraph replay, and the engines end to
end: probe_accumulate, with_head, save / load_engine / ivit_model_open."""
import ctypes
import os

import numpy as np
import pytest

from conftest import golden_scales, load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from ivit_amd.predict import class_map_reference, probe_stats_reference, topk_reference  # noqa: E402
from ivit_amd.probe import Head, ProbeStats  # noqa: E402

_P = ctypes.c_void_p
GUARD_BYTES = 4096
FILL = 0x5A


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


def P(t):
    return None if t is None else _P(t.data_ptr())


def guarded(nbytes, fill=None):
    """(whole buffer, payload view): `nbytes` of payload between two 4 KiB guards filled with 0x5A; the payload zeroed, or holding
    the bytes of `fill`"""
    whole = torch.full((GUARD_BYTES + nbytes + GUARD_BYTES,), FILL, dtype=torch.uint8, device="cuda")
    pay = whole[GUARD_BYTES:GUARD_BYTES + nbytes]
    if fill is None:
        pay.zero_()
    else:
        pay.copy_(torch.from_numpy(np.ascontiguousarray(fill).view(np.uint8).reshape(-1)))
    return whole, pay


def guards_intact(whole, nbytes):
    return bool(((whole[:GUARD_BYTES] == FILL).all() & (whole[GUARD_BYTES + nbytes:] == FILL).all()).item())


class Buffers:
    """the three outputs of a (dim, num_classes), zeroed, each between guard bands"""

    def __init__(self, dim, C):
        self.dim, self.C = dim, C
        self.sizes = (8 * dim * dim, 8 * C * dim, 8 * C)
        self.whole, self.pay = zip(*(guarded(n) for n in self.sizes))

    def ptrs(self):
        return tuple(P(p) for p in self.pay)

    def read(self):
        g, s, c = (p.cpu().numpy().view(np.int64) for p in self.pay)
        return g.reshape(self.dim, self.dim), s.reshape(self.C, self.dim), c

    def intact(self):
        return all(guards_intact(w, n) for w, n in zip(self.whole, self.sizes))


def accumulate(H, x, lab, C, splits, out):
    """one ivit_probe_accumulate of host arrays x int8 [rows, dim], lab int64 [rows] into `out`, the inputs between guard bands too:
    they must come back as they went"""
    rows, dim = x.shape
    xw, xd = guarded(max(rows * dim, 16), x if rows else None)
    lw, ld = guarded(max(8 * rows, 8), lab if rows else None)
    H.call("ivit_probe_accumulate", P(xd), P(ld), rows, dim, C, splits, *out.ptrs())
    torch.cuda.synchronize()
    assert out.intact(), "wrote outside an output"
    assert guards_intact(xw, xd.numel()) and guards_intact(lw, ld.numel())
    if rows:
        assert np.array_equal(xd.cpu().numpy().view(np.int8).reshape(rows, dim), x) and np.array_equal(ld.cpu().numpy().view(np.int64), lab)


def same(got, want, label):
    for name, g, w in zip(("gram", "class_sum", "count"), got, want):
        assert g.dtype == np.int64 and np.array_equal(g, w), (label, name, np.argwhere(g != w)[:4].tolist())


def random_batch(rng, rows, dim, C):
    x = rng.integers(-128, 128, size=(rows, dim)).astype(np.int8)
    x[0, 0], x[-1, -1] = -128, -128
    lab = rng.integers(0, C, size=rows).astype(np.int64)
    if rows >= 31:
        lab[rng.integers(0, rows, size=3)] = -1          # a few rows that take no part
    return x, lab


# ---------------------------------------------------------------- the sweep
@pytest.mark.parametrize("dim", [64, 192, 384, 1024])
def test_probe_accumulate_sweep(H, dim):
    rng = np.random.default_rng(100 + dim)
    for rows in (1, 31, 33, 257):
        for C in (1, 10, 1000):
            (x1, l1), (x2, l2) = random_batch(rng, rows, dim, C), random_batch(rng, rows, dim, C)
            ref1, ref2 = probe_stats_reference(x1, l1, C), probe_stats_reference(x2, l2, C)
            assert np.array_equal(ref1[0], ref1[0].T)
            both = tuple(a + b for a, b in zip(ref1, ref2))
            for splits in (0, 1, 3):
                out = Buffers(dim, C)
                accumulate(H, x1, l1, C, splits, out)
                same(out.read(), ref1, (dim, rows, C, splits, "first call"))
                accumulate(H, x2, l2, C, splits, out)                 # adds, never zeroes
                same(out.read(), both, (dim, rows, C, splits, "second call"))


def test_probe_accumulate_beyond_the_int32_bound(H):
    """131 073 rows of -128: every Gram entry is 131 073 * 16 384 > 2^31, more than an int32 accumulator holds"""
    rows, dim = 131073, 64
    x, lab = np.full((rows, dim), -128, np.int8), np.zeros(rows, np.int64)
    out = Buffers(dim, 1)
    accumulate(H, x, lab, 1, 1, out)
    gram, class_sum, count = out.read()
    assert 131073 * 16384 > 2 ** 31
    assert np.array_equal(gram, np.full((dim, dim), 131073 * 16384, np.int64))
    assert np.array_equal(class_sum, np.full((1, dim), -128 * 131073, np.int64)) and count.tolist() == [131073]


@pytest.mark.parametrize("C", [5, 1000])
def test_probe_accumulate_ignores_labels_outside_the_classes(H, C):
    rng = np.random.default_rng(9)
    rows, dim = 200, 128
    x = rng.integers(-128, 128, size=(rows, dim)).astype(np.int8)
    lab = rng.integers(0, C, size=rows).astype(np.int64)
    lab[:8] = 3
    valid3 = int((lab == 3).sum())
    odd = [-1, C, 2 ** 32 + 3, 2 ** 40, -2 ** 63, 2 ** 63 - 1, 2 ** 32, -(2 ** 32) + 3]
    where = rng.choice(np.arange(8, rows), size=len(odd), replace=False)
    valid3 -= int((lab[where] == 3).sum())
    lab[where] = odd
    out = Buffers(dim, C)
    accumulate(H, x, lab, C, 0, out)
    keep = np.ones(rows, bool)
    keep[where] = False
    want = probe_stats_reference(x[keep], lab[keep], C)             # those rows change nothing ...
    same(out.read(), want, "ignored rows")
    same(out.read(), probe_stats_reference(x, lab, C), "the reference ignores them too")
    assert out.read()[2][3] == valid3 and out.read()[2].sum() == rows - len(odd)      # ... and class 3 is not credited for 2^32 + 3


# ---------------------------------------------------------------- the empty call and the refusals
def test_probe_accumulate_empty_and_refused_calls(H):
    rng = np.random.default_rng(4)
    rows, dim, C = 70, 64, 6
    x, lab = random_batch(rng, rows, dim, C)
    n_g, n_s, n_c = 8 * dim * dim, 8 * C * dim, 8 * C
    inputs = torch.zeros(8 * n_g, dtype=torch.uint8, device="cuda")       # the two inputs far apart in ONE allocation: an output laid over
    xd, ld = inputs[:rows * dim].view(torch.int8).view(rows, dim), inputs[4 * n_g:4 * n_g + 8 * rows].view(torch.int64)     # one reaches no other array
    xd.copy_(torch.from_numpy(x))
    ld.copy_(torch.from_numpy(lab))
    whole, pay = guarded(n_g + n_s + n_c)
    pay.fill_(FILL)
    gram, csum, cnt = pay[:n_g], pay[n_g:n_g + n_s], pay[n_g + n_s:]
    fn = H.lib.ivit_probe_accumulate

    def call(feat=P(xd), labels=P(ld), rows_=rows, dim_=dim, C_=C, splits=0, g=P(gram), s=P(csum), c=P(cnt)):
        return fn(H.h, feat, labels, rows_, dim_, C_, splits, g, s, c)

    INV, UNS = _lib.IVIT_ERR_INVALID, _lib.IVIT_ERR_UNSUPPORTED
    assert call(rows_=0) == _lib.IVIT_OK                          # nothing to do: nothing launched
    for null in ("feat", "labels", "g", "s", "c"):
        assert call(**{null: None}) == INV, null
    assert call(dim_=96) == UNS and call(dim_=0) == UNS and call(dim_=1088) == UNS and call(dim_=32) == UNS
    assert call(rows_=-1) == INV and call(C_=0) == INV and call(C_=65537) == INV and call(splits=-1) == INV and call(splits=65536) == INV
    assert call(feat=_P(xd.data_ptr() + 8), rows_=rows - 1) == INV and b"feat8" in H.lib.ivit_last_error(H.h)
    assert call(labels=_P(ld.data_ptr() + 4), rows_=rows - 1) == INV and call(g=_P(gram.data_ptr() + 4)) == INV
    pairs = [(dict(s=_P(gram.data_ptr() + n_g - 8)), b"gram", b"class_sum"), (dict(c=_P(gram.data_ptr() + 8)), b"gram", b"count"),
             (dict(c=_P(csum.data_ptr() + n_s - 8)), b"class_sum", b"count"), (dict(g=P(xd)), b"feat8", b"gram"),
             (dict(s=_P(xd.data_ptr() + 64)), b"feat8", b"class_sum"), (dict(c=_P(xd.data_ptr() + rows * dim - 8)), b"feat8", b"count"),
             (dict(g=P(ld)), b"labels", b"gram"), (dict(s=P(ld)), b"labels", b"class_sum"), (dict(c=_P(ld.data_ptr() + 8 * rows - 8)), b"labels", b"count")]
    for kw, a, b in pairs:                                            # each overlap, named
        assert call(**kw) == INV, kw
        err = H.lib.ivit_last_error(H.h)
        assert b"overlap" in err and a in err and b in err, err
    torch.cuda.synchronize()
    assert np.all(whole.cpu().numpy() == FILL), "an empty or refused call wrote"
    assert np.array_equal(xd.cpu().numpy(), x) and np.array_equal(ld.cpu().numpy(), lab)
    pay.zero_()
    assert call() == _lib.IVIT_OK                                 # and the same arguments, unharmed, are accepted
    torch.cuda.synchronize()
    got = tuple(t.cpu().numpy().view(np.int64) for t in (gram, csum, cnt))
    same((got[0].reshape(dim, dim), got[1].reshape(C, dim), got[2]), probe_stats_reference(x, lab, C), "after the refusals")
    assert guards_intact(whole, pay.numel())


# ---------------------------------------------------------------- hipGraph
def test_probe_accumulate_captured_in_a_graph_replays_on_new_features_and_labels():
    rng = np.random.default_rng(12)
    rows, dim, C = 300, 192, 10
    (x1, l1), (x2, l2) = random_batch(rng, rows, dim, C), random_batch(rng, rows, dim, C)
    stream = torch.cuda.Stream()
    h2 = _lib.Handle(0, stream.cuda_stream)
    xb, lb = torch.from_numpy(x1).cuda(), torch.from_numpy(l1).cuda()
    stats = ProbeStats(dim, C, "cuda:0")
    args = (P(xb), P(lb), rows, dim, C, 0) + tuple(P(t) for t in stats.tensors())
    with torch.cuda.stream(stream):                               # eager once, into buffers of its own: the code is loaded outside the capture
        h2.call("ivit_probe_accumulate", *(args[:6] + tuple(P(t) for t in ProbeStats(dim, C, "cuda:0").tensors())))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
        h2.call("ivit_probe_accumulate", *args)
    torch.cuda.synchronize()
    assert not any(a.any() for a in stats.numpy())                # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    ref1, ref2 = probe_stats_reference(x1, l1, C), probe_stats_reference(x2, l2, C)
    same(stats.numpy(), ref1, "first replay")
    xb.copy_(torch.from_numpy(x2))                                # a second batch in the same buffers
    lb.copy_(torch.from_numpy(l2))
    graph.replay()
    torch.cuda.synchronize()
    same(stats.numpy(), tuple(a + b for a, b in zip(ref1, ref2)), "second replay")


def test_probe_stats_add_merge_zero():
    rng = np.random.default_rng(2)
    x, lab = random_batch(rng, 90, 128, 7)
    xd, ld = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()
    a, b = ProbeStats(128, 7, "cuda:0"), ProbeStats(128, 7, "cuda:0")
    a.add(xd[:50], ld[:50])
    b.add(xd[50:], ld[50:]).add(xd[:0], ld[:0])
    same(a.merge(b).numpy(), probe_stats_reference(x, lab, 7), "merge")
    assert not any(t.any() for t in a.zero_().numpy())


# ---------------------------------------------------------------- end to end on the engines
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
    return cfg, eng


@pytest.mark.parametrize("fname", ["micro_vit_b2.npz", "micro_swin_b2.npz"])
def test_probe_accumulate_and_with_head_end_to_end(fname, tmp_path):
    cfg, eng = _engine(fname)
    swin = str(load_golden(fname)["cfg_name"]) in iv.SWIN_CONFIGS
    B, C = 5, 4
    assert eng.num_features == 64
    images = torch.from_numpy(iv.make_images_int8(cfg, B, seed=41)).cuda()
    labels = torch.tensor([0, 3, 1, 7, 3], dtype=torch.int64, device="cuda")          # 7: ignored
    before = eng.forward(images, copy=True)
    feat8 = eng.features(images, copy=True)[0]
    f8 = feat8.cpu().numpy()

    stats = ProbeStats(eng.num_features, C, eng.device)
    got8 = eng.probe_accumulate(images, labels, stats)
    assert torch.equal(got8, feat8)
    same(stats.numpy(), probe_stats_reference(f8, labels.cpu().numpy(), C), "probe_accumulate")
    eng.probe_accumulate(images, labels, stats, nslices=2)
    same(stats.numpy(), tuple(2 * a for a in probe_stats_reference(f8, labels.cpu().numpy(), C)), "a second batch")

    rng = np.random.default_rng(5)
    s_feat = eng.feature_scale_host()
    head = Head.from_float(rng.standard_normal((C, 64)).astype(np.float32) * 0.05, rng.standard_normal(C).astype(np.float32), s_feat)
    new = eng.with_head(head)
    assert type(new) is type(eng) and new.cfg.num_classes == C and eng.cfg.num_classes == 10 and new.num_features == 64
    assert new.feature_scale_host() == s_feat and new.input_scale_host() == eng.input_scale_host()
    assert np.array_equal(new.head_scale_host().view(np.uint32), head.scale.view(np.uint32))
    want = head.logits_reference(f8)
    logits = new.forward(images, copy=True)
    assert logits.dtype == torch.int32 and logits.shape == (B, C) and np.array_equal(logits.cpu().numpy(), want)
    assert torch.equal(new.features(images)[0], feat8)            # the backbone is the same
    ri, rv = topk_reference(want, head.scale, C)
    idx, val = new.predict(images, k=C, copy=True)
    assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(val.cpu().numpy().view(np.uint32), rv.view(np.uint32))
    assert np.array_equal(rv, np.take_along_axis(want.astype(np.float32) * head.scale[None, :], ri.astype(np.int64), axis=1))

    path = new.save(str(tmp_path / "probe.ivit"))
    again = iv.load_engine(path)
    assert again.cfg.num_classes == C and np.array_equal(again.forward(images).cpu().numpy(), want)
    h = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    m = _P()
    assert h.lib.ivit_model_open(h.h, os.fsencode(path), 2, ctypes.byref(m)) == _lib.IVIT_OK and m.value, h.lib.ivit_last_error(h.h)
    info = _lib.ModelInfo()
    assert h.lib.ivit_model_get_info(m, ctypes.byref(info)) == _lib.IVIT_OK
    assert (info.num_classes, info.num_features) == (C, 64) and np.float32(info.s_features) == np.float32(s_feat)
    assert h.lib.ivit_model_close(m) == _lib.IVIT_OK
    h.close()

    if swin:                                                      # the class maps' unit follows the new head
        class_scale = (np.float32(eng.token_scale_host()) * head.weight_scale).astype(np.float32)
        assert np.array_equal(new.class_scale.cpu().numpy().view(np.uint32), class_scale.view(np.uint32))
        assert np.array_equal(again.class_scale.cpu().numpy().view(np.uint32), class_scale.view(np.uint32))
        ci, cv, tok8, cam32, maps = new.class_map(images, k=2, copy=True)
        assert np.array_equal(ci.cpu().numpy(), ri[:, :2])
        wcam, wmap = class_map_reference(tok8.cpu().numpy(), head.w8, ri[:, :2], class_scale)
        g = maps.shape[-1]
        assert np.array_equal(cam32.cpu().numpy(), wcam) and np.array_equal(maps.cpu().numpy().view(np.uint32), wmap.reshape(B, 2, g, g).view(np.uint32))

    with pytest.raises(iv.IvitError):                             # another width, another features' scale
        eng.with_head(Head.from_float(np.zeros((C, 128), np.float32), np.zeros(C, np.float32), s_feat))
    with pytest.raises(iv.IvitError):
        eng.with_head(Head.from_float(head.weight, head.bias, s_feat * 2))
    assert torch.equal(eng.forward(images), before)               # the original engine is what it was
