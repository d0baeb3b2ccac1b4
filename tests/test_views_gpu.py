"""Image views on the device (include/ivit_views.h): ivit_view_resize_u8_pil and ivit_view_transform_u8 against Pillow's recorded
bytes (tests/golden/pil_views.npz: every byte, no tolerance) and against `views.views_reference` on the forms the fixture's small
images cannot reach, their memory and overlap contracts on the arena harness of tests/abi_cases.py, their refusals;
ivit_logits_view_sum against `predict.view_sum_reference`; and the engines' predict_views / score_views / evaluate(views=) end to end.

The fixture's views have crops of 16, 7 and 1 (a mirrored view needs an odd and an even crop, and crop 1 is a class of its own) and a
launch has ONE crop: "all views in one launch" is one launch per crop, all views of that crop together."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import load_golden, golden_scales

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import abi_cases as A  # noqa: E402
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from ivit_amd import preprocess as pp  # noqa: E402
from ivit_amd import views as vw  # noqa: E402
from ivit_amd.predict import evaluate, score_reference, topk_reference, view_scale_reference, view_sum_reference  # noqa: E402
from pil_fixture import case_ids, fixture  # noqa: E402
from pil_views_fixture import group_ids, views_fixture  # noqa: E402
from pil_views_fixture import entry_args as _args  # noqa: E402    -> (entry, argument list in abi_cases' form, the host tables)

GROUPS = range(len(group_ids()))
ARGNAMES = {name: [p.name for p in _lib.VIEWS_ABI.functions[name].params[1:]] for name in _lib.VIEWS_ABI.functions}


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _packed():
    """all images of the fixture as ONE ragged batch on the device: the fixture's views name them by index"""
    return pp.pack_images(views_fixture()[1], "cuda")


def _nq(u8, scale):
    """the existing entry on a uint8 [B, S, S, 3] array -> int8 [B, 3, S, S] (numpy)"""
    return pp.normalize_quantize(torch.from_numpy(np.ascontiguousarray(u8)).cuda(), scale).cpu().numpy()


def _gen(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---------------------------------------------------------------- outputs
@pytest.mark.parametrize("k", GROUPS, ids=group_ids())
def test_all_fixture_views_in_one_launch_equal_pil_bytes(k):
    crop, views, want = views_fixture()[2][k]
    got = vw.view_resize(_packed(), views, crop).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), [int((a != b).sum()) for a, b in zip(got, want)]


@pytest.mark.parametrize("scale", [0.03, 0.004], ids=["no-saturation", "saturating"])
@pytest.mark.parametrize("k", GROUPS, ids=group_ids())
def test_view_transform_equals_normalize_quantize_of_pil_bytes(k, scale):
    crop, views, want = views_fixture()[2][k]
    ref = _nq(want, scale)
    if scale == 0.004:
        if crop == 16:                  # the group holds a copied box of a saturated 0 / 255 image: both ends of the table are reached
            assert ref.max() == 127 and ref.min() == -128
    else:
        assert -128 < ref.min() and ref.max() < 127
    got = vw.view_transform(_packed(), views, scale, crop).cpu().numpy()
    assert got.dtype == np.int8 and got.shape == (len(views), 3, crop, crop)
    assert np.array_equal(got, ref), int((got != ref).sum())


@pytest.mark.parametrize("k", range(len(case_ids())), ids=case_ids())
def test_center_views_equal_the_eval_transform_byte_for_byte(k):
    _, images, cases = fixture()
    size, crop, idx, want = cases[k]
    batch = pp.pack_images([images[i] for i in idx], "cuda")
    views = vw.center_views(batch, size, crop)
    got = vw.view_resize(batch, views, crop)
    assert torch.equal(got, pp.resize_center_crop_pil(batch, size, crop)) and np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(vw.view_transform(batch, views, 0.03, crop), pp.eval_transform_pil(batch, 0.03, size, crop))


FORMS = [(330, 420, 300, 290, "two column chunks (crop > 256)"),
         (200, 310, 24, 22, "a chunk narrowed to the tap table (ksize_h 37)"),
         (1200, 1400, 40, 36, "streaming, column chunks of 33, two bands"),
         (1030, 1026, 1, 1, "coefficients per tap (ksize_h 4097)")]


@functools.lru_cache(maxsize=None)
def _form(i):
    """-> (images, view table without flips, reference bytes): the box (bh x bw) lies INSIDE a larger image at an odd offset, so the
    row stride differs from the box's width; a small tiled view of a second image rides in the same launch"""
    bh, bw, size, crop, _ = FORMS[i]
    rng = np.random.Generator(np.random.PCG64(11 + i))
    ims = [_gen(rng, bh + 9, bw + 7), _gen(rng, 37, 53)]
    Hr, Wr = pp.resized_size(bh, bw, size)
    views = vw.make_views([(0, 3, 5, bw, bh, Wr, Hr, pp.crop_offset(Wr, crop), pp.crop_offset(Hr, crop), 0),
                           (1, 1, 2, 40, 30, crop + 3, crop + 2, 2, 1, 0)])
    return ims, views, vw.views_reference(ims, views, crop)


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("i", range(len(FORMS)), ids=[f"{f[0]}x{f[1]}" for f in FORMS])
def test_forms_beyond_the_fixture_equal_the_reference(i, flip):
    ims, views, want = _form(i)
    crop, what = FORMS[i][3], FORMS[i][4]
    views = views.copy()
    views["flip"] = flip
    if flip:
        want = want[:, :, ::-1]
    got = vw.view_resize(pp.pack_images(ims, "cuda"), views, crop).cpu().numpy()
    assert np.array_equal(got, want), (what, [int((a != b).sum()) for a, b in zip(got, want)])


def test_a_view_depends_on_no_byte_outside_its_box():
    rng = np.random.Generator(np.random.PCG64(21))
    im = _gen(rng, 80, 90)
    x0, y0, bw, bh = 7, 9, 40, 50
    views = vw.make_views([(0, x0, y0, bw, bh, 20, 24, 3, 5, 0), (0, x0, y0, bw, bh, 61, 77, 45, 61, 1), (0, x0, y0, bw, bh, 40, 16, 12, 0, 1),
                           (0, x0, y0, bw, bh, 17, 50, 0, 17, 0)])
    first = vw.view_resize(pp.pack_images([im], "cuda"), views, 16).cpu().numpy()
    other = _gen(rng, 80, 90)
    other[y0:y0 + bh, x0:x0 + bw] = im[y0:y0 + bh, x0:x0 + bw]
    assert (other != im).sum() > 1000
    second = vw.view_resize(pp.pack_images([other], "cuda"), views, 16).cpu().numpy()
    assert np.array_equal(first, second) and np.array_equal(first, vw.views_reference([im], views, 16))


# ---------------------------------------------------------------- memory contract
@pytest.mark.parametrize("nchw", [False, True], ids=["hwc", "nchw"])
@pytest.mark.parametrize("k", GROUPS, ids=group_ids())
def test_memory_contract(H, k, nchw):
    """every array in its own [1 MiB guard | payload | 1 MiB guard] arena: every output byte written, the guards untouched under
    two fills, the outputs unchanged when the guards of pixels (where an edge tap would over-read) and of BOTH tables go from 0x7F
    to 0xFF, equal to PIL's bytes; and the same with pixels, then the output, one element off 16-byte alignment"""
    _, images, groups = views_fixture()
    crop, views, want = groups[k]
    name, args, keep = _args(images, views, crop, nchw)
    fn, mem = getattr(H.lib, name), A.TorchMem()
    got = A.check_contract(fn, H.h, args, mem, what=name)
    ref = _nq(want, 0.03).view(np.uint8) if nchw else want
    assert np.array_equal(got[0], ref.reshape(-1))
    plain = A.plain_outputs(fn, H.h, args, mem)
    assert np.array_equal(plain[0], got[0])
    for idx in (0, len(args) - 1):
        A.check_alignment(fn, H, args, mem, None, idx, "exact", got, name)


def _small_case(rng):
    ims = [_gen(rng, 40, 50), _gen(rng, 30, 64), _gen(rng, 44, 33)]
    views = vw.make_views([(0, 2, 3, 30, 20, 24, 22, 1, 0, 0), (2, 0, 0, 33, 44, 21, 28, 0, 5, 1), (1, 10, 4, 50, 26, 50, 30, 13, 7, 0),
                           (0, 0, 0, 50, 40, 20, 20, 0, 0, 1)])
    return ims, views


@pytest.mark.parametrize("nchw", [False, True], ids=["hwc", "nchw"])
def test_overlap_contract(H, nchw):
    """the output laid over the pixel blob, over the device image table or over the device view table is refused before anything is
    launched, with both names in the message and no byte changed; touching arrays give the bytes of the plain call"""
    ims, views = _small_case(np.random.Generator(np.random.PCG64(5)))
    name, args, keep = _args(ims, views, 20, nchw)
    A.check_overlap(getattr(H.lib, name), H, args, A.TorchMem(), None, name, inplace={}, inputs=(0, 3, 6), argnames=ARGNAMES[name])


# ---------------------------------------------------------------- refusals
def _refused(H, name, args, word):
    mem = A.TorchMem()
    arenas = A._place(mem, [a for a in args])
    outs = A._run_placed(getattr(H.lib, name), H.h, args, arenas, mem, 0xA5, 0x7F, None, status=_lib.IVIT_ERR_INVALID)
    msg = H.lib.ivit_last_error(H.h).decode()
    assert word in msg, msg
    for pay, front, back in outs:
        assert not front and not back and (pay == 0xA5).all(), "a refused call wrote its output"


@pytest.mark.parametrize("nchw", [False, True], ids=["hwc", "nchw"])
def test_refusals_name_the_view_and_launch_nothing(H, nchw):
    rng = np.random.Generator(np.random.PCG64(3))
    ims, views = _small_case(rng)
    crop = 20
    name, good, _ = _args(ims, views, crop, nchw)
    assert A.check_contract(getattr(H.lib, name), H.h, good, A.TorchMem())
    # view 1 is (image 2: 44 x 33; box 0, 0, 33, 44; resized to 21 x 28; window 0, 5; mirrored)
    table = (("image", 3, "view 1: image outside"), ("image", -1, "view 1: image outside"),
             ("x0", 1, "view 1: box outside"),                     # past the right edge by one pixel
             ("y0", 1, "view 1: box outside"),                     # past the bottom edge by one pixel
             ("x0", -1, "view 1: box outside"), ("bw", 0, "view 1: empty box"), ("bh", -2, "view 1: empty box"),
             ("rw", 0, "view 1: resized size"), ("rw", 65537, "view 1: resized size"), ("rh", 0, "view 1: resized size"),
             ("left", 2, "view 1: window outside"),                # 2 + 20 > 21: past rw
             ("top", 9, "view 1: window outside"), ("left", -1, "view 1: window outside"),
             ("flip", 2, "view 1: flip"), ("flip", -1, "view 1: flip"))
    for field, value, word in table:
        bad = views.copy()
        bad[field][1] = value
        _, args, _keep = _args(ims, bad, crop, nchw)
        _refused(H, name, args, word)
    bad = views.copy()
    bad["rw"][3] = 19                                              # the crop itself larger than the resized box: view 3
    _refused(H, name, _args(ims, bad, crop, nchw)[1], "view 3: window outside")
    # the image table's checks are those of the ragged entries
    args = list(good)
    args[1] = good[1] - 1
    _refused(H, name, args, "image 2: reaches past pixels_bytes")
    _, args, (desc, _v) = _args(ims, views, crop, nchw)
    desc["h"][1] = 0
    _refused(H, name, args, "image 1: non-positive side")
    # B = 0, V < 0, a non-positive crop
    for pos, value in ((4, 0), (4, -1), (7, -1), (8, 0)):
        args = list(good)
        args[pos] = value
        _refused(H, name, args, "bad arguments")
    # null pointers: pixels, the host tables, the device tables, the output
    for pos in (0, 2, 3, 5, 6, len(good) - 1):
        args = list(good)
        args[pos] = None
        _refused(H, name, args, "bad arguments")
    if nchw:
        for pos, value in ((9, None), (10, None), (11, 0.0), (10, ("host", np.array([0.2, 0.0, 0.2], np.float32)))):
            args = list(good)
            args[pos] = value
            _refused(H, name, args, "zero std" if isinstance(value, tuple) else "bad arguments")


@pytest.mark.parametrize("nchw", [False, True], ids=["hwc", "nchw"])
def test_no_views_launch_nothing(H, nchw):
    ims, views = _small_case(np.random.Generator(np.random.PCG64(4)))
    name, args, _ = _args(ims, views, 20, nchw)
    for null_tables in (False, True):
        a = list(args)
        a[7] = 0                                                   # V = 0: the output keeps its fill, IVIT_OK
        if null_tables:
            a[5] = a[6] = None
        mem = A.TorchMem()
        arenas = A._place(mem, a)
        outs = A._run_placed(getattr(H.lib, name), H.h, a, arenas, mem, 0xA5, 0x7F, None, status=_lib.IVIT_OK)
        for pay, front, back in outs:
            assert not front and not back and (pay == 0xA5).all()
    batch = pp.pack_images(ims, "cuda")
    assert vw.view_resize(batch, views[:0], 20).shape == (0, 20, 20, 3) and vw.view_transform(batch, views[:0], 0.03, 20).shape == (0, 3, 20, 20)


# ---------------------------------------------------------------- the sum of the views' logits
def _run_sum(H, acc, groups, views, off=0, status=0):
    """ivit_logits_view_sum on a host array; `off`: int32 elements both device pointers lie behind a 256-byte boundary; one guard
    row behind the output must stay untouched"""
    ncls = acc.shape[1]
    src = torch.zeros(acc.size + off + 4, dtype=torch.int32, device="cuda")
    src[off:off + acc.size] = torch.from_numpy(acc.reshape(-1)).cuda()
    out = torch.full(((groups + 1) * ncls + off,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    st = H.lib.ivit_logits_view_sum(H.h, ctypes.c_void_p(src.data_ptr() + 4 * off), groups, views, ncls, ctypes.c_void_p(out.data_ptr() + 4 * off))
    assert st == status, (st, H.lib.ivit_last_error(H.h).decode())
    got = out.cpu().numpy()
    assert (got[:off] == 0x5A5A5A5A).all() and (got[off + groups * ncls:] == 0x5A5A5A5A).all(), "wrote outside its output"
    return got[off:off + groups * ncls].reshape(groups, ncls)


@pytest.mark.parametrize("groups,views,ncls,off", [(3, 5, 10, 0), (2, 10, 1000, 0), (1, 1, 7, 0), (4, 64, 13, 0), (2, 3, 9, 1), (5, 7, 64, 0), (3, 2, 64, 1)],
                         ids=lambda v: str(v))
def test_logits_view_sum_equals_reference(H, groups, views, ncls, off):
    rng = np.random.default_rng(groups * 1000 + views)
    acc = rng.integers(-2**31, 2**31, size=(groups * views, ncls), dtype=np.int64).astype(np.int32)
    acc[:, 1:] >>= 8                                                # column 0 spans all of int32: with more than one view it saturates
    acc[:views, 0] = np.iinfo(np.int32).max                          # group 0, column 0: the upper end
    if groups > 1:
        acc[views:2 * views, 0] = np.iinfo(np.int32).min             # group 1, column 0: the lower end
    want = view_sum_reference(acc, views)
    if views > 1:
        assert want[0, 0] == np.iinfo(np.int32).max and (groups == 1 or want[1, 0] == np.iinfo(np.int32).min)
    assert np.array_equal(_run_sum(H, acc, groups, views, off), want)


def test_logits_view_sum_edges_and_refusals(H):
    acc = np.arange(60, dtype=np.int32).reshape(6, 10)
    assert _run_sum(H, acc[:0], 0, 3).shape == (0, 10)              # groups = 0: nothing launched, nothing written
    for views in (0, 65, -1):
        _run_sum(H, acc, 0, views, status=_lib.IVIT_ERR_INVALID)
        assert "views must be in 1 .. 64" in H.lib.ivit_last_error(H.h).decode()
    buf = torch.zeros(256, dtype=torch.int32, device="cuda")
    P = lambda o: ctypes.c_void_p(buf.data_ptr() + 4 * o)          # noqa: E731
    for o in (0, 10, 59):                                           # out over logits [0, 60): refused, both names in the message
        assert H.lib.ivit_logits_view_sum(H.h, P(0), 2, 3, 10, P(o)) == _lib.IVIT_ERR_INVALID
        msg = H.lib.ivit_last_error(H.h).decode()
        assert "overlap" in msg and "logits" in msg and "out" in msg
    assert H.lib.ivit_logits_view_sum(H.h, P(0), 2, 3, 10, P(60)) == _lib.IVIT_OK          # touching arrays are fine
    assert H.lib.ivit_logits_view_sum(H.h, P(20), 2, 3, 10, P(0)) == _lib.IVIT_OK
    for a, b in ((None, P(0)), (P(0), None)):
        assert H.lib.ivit_logits_view_sum(H.h, a, 2, 3, 10, b) == _lib.IVIT_ERR_INVALID
    assert H.lib.ivit_logits_view_sum(H.h, P(0), 2, 3, 0, P(100)) == _lib.IVIT_ERR_INVALID
    assert H.lib.ivit_logits_view_sum(H.h, P(0), -1, 3, 10, P(100)) == _lib.IVIT_ERR_INVALID
    torch.cuda.synchronize()
    assert not buf.any()


# ---------------------------------------------------------------- end to end
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


def _assert_nll(got, want):
    """the bound of include/ivit_eval.h on two orders of the fp64 sum, as tests/test_score_gpu.py applies it"""
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("fname", ["micro_vit_b2.npz", "micro_swin_b2.npz"])
def test_ten_crop_end_to_end(fname):
    """a ten-crop of three fixture images at the model's input size: predict_views / score_views / evaluate(views=10) against the
    numpy statements on engine.forward's logits of the same int8 views"""
    cfg, eng = _engine(fname)
    crop, V = cfg.img_size, 10
    size = crop + 5
    images = [views_fixture()[1][i] for i in (20, 21, 24)]             # 40 x 44, 50 x 38, 70 x 41
    n = len(images)
    batch = pp.pack_images(images, "cuda")
    s_in = eng.input_scale_host()
    table = vw.ten_crop_views(batch, size, crop)
    q = vw.view_transform(batch, table, s_in, crop)
    assert q.shape == (n * V, 3, crop, crop)
    assert np.array_equal(q.cpu().numpy(), _nq(vw.views_reference(images, table, crop), s_in))
    logits = eng.forward(q, copy=True).cpu().numpy()
    total = view_sum_reference(logits, V)
    scale_v = view_scale_reference(eng.head_scale_host(), V)
    assert np.array_equal(eng.view_scale(V).cpu().numpy(), scale_v)
    k = min(5, cfg.num_classes)
    want_idx, want_val = topk_reference(total, scale_v, k)
    for nslices in (1, 2):
        idx, val, got_total = eng.predict_views(q, views=V, k=k, nslices=nslices)
        assert idx.shape == val.shape == (n, k) and got_total.shape == (n, cfg.num_classes)
        assert np.array_equal(got_total.cpu().numpy(), total) and np.array_equal(idx.cpu().numpy(), want_idx)
        assert np.array_equal(val.cpu().numpy().view(np.uint32), want_val.view(np.uint32))
    ranks = np.array([0, min(2, cfg.num_classes - 1), min(4, cfg.num_classes - 1)])
    order = topk_reference(total, scale_v, min(16, cfg.num_classes))[0]
    labels = order[np.arange(n), ranks].astype(np.int64)
    d_labels = torch.from_numpy(labels).cuda()
    want_rank, want_nll = score_reference(total, scale_v, labels)
    assert want_rank.tolist() == ranks.tolist()
    rank, nll = eng.score_views(q, d_labels, views=V)
    assert np.array_equal(rank.cpu().numpy(), want_rank)
    _assert_nll(nll.cpu().numpy(), want_nll)
    # what raises before anything runs
    for bad in (0, 65, 4):                                             # 30 images are no multiple of 4
        with pytest.raises(ValueError):
            eng.predict_views(q, views=bad)
        with pytest.raises(ValueError):
            eng.score_views(q, d_labels, views=bad)
    # evaluate: ragged batches of 2 and 1 images, ten views each
    def tf(rag):
        return vw.view_transform(rag, vw.ten_crop_views(rag, size, crop), s_in, crop)
    batches = [(batch[a:a + 2], d_labels[a:a + 2]) for a in range(0, n, 2)]
    out = evaluate(eng, batches, topk=(1, 3, 5), transform=tf, views=V)
    expect = {j: int((want_rank < j).sum()) for j in (1, 3, 5)}
    assert out["n"] == n and out["correct"] == expect
    out = evaluate(eng, batches, topk=(1, 3, 5), transform=tf, views=V, loss=True)
    assert out["n"] == n and out["correct"] == expect
    np.testing.assert_allclose(out["loss"], want_nll.mean(), rtol=1e-12, atol=1e-9)
    # views = 1 is evaluate as it was: the centre view of every image, one label per image
    def tf1(rag):
        return pp.eval_transform_pil(rag, s_in, size, crop)
    plain = evaluate(eng, batches, topk=(1, 5), transform=tf1)
    assert evaluate(eng, batches, topk=(1, 5), transform=tf1, views=1) == plain
    q1 = tf1(batch)
    r1 = score_reference(eng.forward(q1, copy=True).cpu().numpy(), eng.head_scale_host(), labels)[0]
    assert plain["n"] == n and plain["correct"] == {1: int((r1 < 1).sum()), 5: int((r1 < 5).sum())}
    with_loss = evaluate(eng, batches, topk=(1, 5), transform=tf1, loss=True, views=1)
    assert with_loss == evaluate(eng, batches, topk=(1, 5), transform=tf1, loss=True) and with_loss["correct"] == plain["correct"]
