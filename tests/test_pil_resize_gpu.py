"""The PIL-exact ragged front end on the device: ivit_resize_center_crop_u8_pil and ivit_eval_transform_u8 against PIL's recorded
bytes (tests/golden/pil_resize.npz: every byte, no tolerance), their memory contract on the arena harness of tests/abi_cases.py,
their refusals, the forms of the kernel the fixture's small images cannot reach, and evaluate() end to end."""
import numpy as np
import pytest

from conftest import load_golden, golden_scales

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import abi_cases as A  # noqa: E402
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from ivit_amd import preprocess as pp  # noqa: E402
from ivit_amd.predict import evaluate  # noqa: E402
from pil_fixture import case_ids, fixture  # noqa: E402
from pil_fixture import entry_args as _args  # noqa: E402    -> (entry, argument list in abi_cases' form, keep-alive)

CASES = range(len(case_ids()))


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


def _case(k):
    _, images, cases = fixture()
    size, crop, idx, want = cases[k]
    return [images[i] for i in idx], size, crop, want


def _nq(u8, scale):
    """the existing entry on a uint8 [B, S, S, 3] array -> int8 [B, 3, S, S] (numpy)"""
    return pp.normalize_quantize(torch.from_numpy(np.ascontiguousarray(u8)).cuda(), scale).cpu().numpy()


# ---------------------------------------------------------------- outputs
@pytest.mark.parametrize("k", CASES, ids=case_ids())
def test_ragged_batch_equals_pil_bytes(k):
    """the whole case in ONE call, and image by image (B = 1), equal PIL's bytes"""
    ims, size, crop, want = _case(k)
    batch = pp.pack_images(ims, "cuda")
    got = pp.resize_center_crop_pil(batch, size, crop).cpu().numpy()
    assert got.shape == want.shape
    assert np.array_equal(got, want), [int((a != b).sum()) for a, b in zip(got, want)]
    for i in range(len(ims)):
        one = pp.resize_center_crop_pil(batch[i:i + 1], size, crop).cpu().numpy()
        assert np.array_equal(one[0], want[i]), (i, int((one[0] != want[i]).sum()))


@pytest.mark.parametrize("scale", [0.03, 0.004], ids=["no-saturation", "saturating"])
@pytest.mark.parametrize("k", CASES, ids=case_ids())
def test_eval_transform_equals_normalize_quantize_of_pil_bytes(k, scale):
    ims, size, crop, want = _case(k)
    ref = _nq(want, scale)
    if scale == 0.004:
        if k == 0:                      # saturated 0 / 255 images at a mild scale: both ends of the table are reached
            assert ref.max() == 127 and ref.min() == -128
    else:
        assert -128 < ref.min() and ref.max() < 127
    got = pp.eval_transform_pil(pp.pack_images(ims, "cuda"), scale, size, crop).cpu().numpy()
    assert got.dtype == np.int8 and got.shape == (len(ims), 3, crop, crop)
    assert np.array_equal(got, ref), int((got != ref).sum())


def _gen(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("h,w,size,crop,what", [
    (330, 420, 300, 290, "two column chunks (crop > 256)"),
    (200, 310, 24, 22, "a chunk narrowed to the tap table (ksize_h 37)"),
    (1200, 1400, 40, 36, "streaming, column chunks of 33, two bands"),
    (1030, 1026, 1, 1, "coefficients per tap (ksize_h > 4096)"),
])
def test_forms_beyond_the_fixture_equal_the_reference(h, w, size, crop, what):
    """the fixture's images are small; these reach the column-chunk loop, the narrowed chunk, the streaming form over several
    sub-bands and the per-tap coefficients.  The reference is the numpy statement, itself pinned to PIL on the CPU."""
    rng = np.random.Generator(np.random.PCG64(11))
    ims = [_gen(rng, h, w), _gen(rng, 37, 53)]                   # a small tiled image in the same launch
    want = pp.pil_resize_center_crop_reference(ims, size, crop)
    got = pp.resize_center_crop_pil(pp.pack_images(ims, "cuda"), size, crop).cpu().numpy()
    assert np.array_equal(got, want), (what, [int((a != b).sum()) for a, b in zip(got, want)])


# ---------------------------------------------------------------- memory contract
@pytest.mark.parametrize("nchw", [False, True], ids=["hwc", "nchw"])
@pytest.mark.parametrize("k", CASES, ids=case_ids())
def test_memory_contract(H, k, nchw):
    """every array in its own [1 MiB guard | payload | 1 MiB guard] arena: every output byte written, the guards untouched under
    two fills, the outputs unchanged when the guards of pixels (where the edge taps would over-read) and of the descriptor table go
    from 0x7F to 0xFF, equal to PIL's bytes; and the same with pixels, then the output, one element off 16-byte alignment"""
    ims, size, crop, want = _case(k)
    name, args, keep = _args(ims, size, crop, nchw)
    fn, mem = getattr(H.lib, name), A.TorchMem()
    got = A.check_contract(fn, H.h, args, mem, what=name)
    ref = _nq(want, 0.03).view(np.uint8) if nchw else want
    assert np.array_equal(got[0], ref.reshape(-1))
    plain = A.plain_outputs(fn, H.h, args, mem)
    assert np.array_equal(plain[0], got[0])
    for idx in (0, len(args) - 1):
        A.check_alignment(fn, H, args, mem, None, idx, "exact", got, name)


@pytest.mark.parametrize("nchw", [False, True], ids=["hwc", "nchw"])
def test_overlap_contract(H, nchw):
    """include/ivit.h, overlapping arguments, for the two ragged entries (they are in no table of abi_cases): the output laid over
    the pixel blob or over the device descriptor table is refused before anything is launched, with both names in the message and no
    byte changed; touching arrays give the bytes of the plain call.  Three images of different sizes, the placements of
    abi_cases.overlap_placements inside one allocation of the test's own."""
    rng = np.random.Generator(np.random.PCG64(5))
    ims = [_gen(rng, 40, 50), _gen(rng, 30, 64), _gen(rng, 44, 33)]
    name, args, keep = _args(ims, 24, 20, nchw)
    A.check_overlap(getattr(H.lib, name), H, args, A.TorchMem(), None, name, name=name[len("ivit_"):], inputs=(0, 3), inplace={})


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
def test_refusals_launch_nothing(H, nchw):
    rng = np.random.Generator(np.random.PCG64(3))
    ims = [_gen(rng, 40, 50), _gen(rng, 30, 64), _gen(rng, 44, 33)]
    name, good, desc = _args(ims, 24, 20, nchw)
    # crop larger than a resized side: image 0 is 24 x 30 resized, 26 > 24
    _, args, _d = _args(ims, 24, 26, nchw)
    _refused(H, name, args, "image 0: crop larger")
    _, args, _d = _args([ims[0], _gen(rng, 60, 20)], 20, 20, nchw)          # fine: 60 x 20 at size 20, crop 20
    assert A.check_contract(getattr(H.lib, name), H.h, args, A.TorchMem())
    # a record reaching past pixels_bytes: image 2, by one byte
    args = list(good)
    args[1] = good[1] - 1
    _refused(H, name, args, "image 2: reaches past pixels_bytes")
    # a non-positive side, a negative offset
    for field, value, word in (("h", 0, "image 1: non-positive side"), ("w", -3, "image 1: non-positive side"), ("offset", -1, "image 1: negative offset")):
        _, args, d = _args(ims, 24, 20, nchw)
        d[field][1] = value
        _refused(H, name, args, word)
    # B = 0, a non-positive size or crop
    for pos, value in ((4, 0), (4, -1), (5, 0), (6, 0)):
        args = list(good)
        args[pos] = value
        _refused(H, name, args, "bad arguments")
    # null pointers: pixels, the host table, the device table, the output
    for pos in (0, 2, 3, len(good) - 1):
        args = list(good)
        args[pos] = None
        _refused(H, name, args, "bad arguments")
    if nchw:
        for pos, value in ((7, None), (8, None), (9, 0.0), (8, ("host", np.array([0.2, 0.0, 0.2], np.float32)))):
            args = list(good)
            args[pos] = value
            _refused(H, name, args, "zero std" if isinstance(value, tuple) else "bad arguments")


# ---------------------------------------------------------------- end to end
def test_evaluate_over_ragged_batches_equals_the_engine_on_pil_bytes():
    """a micro-ViT (32 px input) over the fixture's five images of the (36, 32) case, in ragged batches of 2 through
    eval_transform_pil, against the same engine on normalize_quantize(PIL's recorded bytes): same logits, same hit counts"""
    from ivit_amd.engine import ViTEngine
    g = load_golden("micro_vit_b2.npz")
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    eng = ViTEngine.from_float(cfg, iv.make_vit_weights(cfg, int(g["seed"])), golden_scales(g))
    s_in = eng.f32["s_in"]
    k = case_ids().index(f"size36-crop{cfg.img_size}")
    ims, size, crop, want = _case(k)
    n = len(ims)
    q_ref = pp.normalize_quantize(torch.from_numpy(want).cuda(), s_in)
    logits_ref = eng.forward(q_ref).cpu().numpy().copy()
    order = eng.predict(q_ref, k=6, copy=True)[0].cpu().numpy()
    ranks = np.array([(0, 2, 5)[i % 3] for i in range(n)])
    labels = torch.from_numpy(order[np.arange(n), ranks].astype(np.int64))
    expect = {1: int((ranks < 1).sum()), 5: int((ranks < 5).sum())}
    ref_out = evaluate(eng, [(q_ref[a:a + 2], labels[a:a + 2]) for a in range(0, n, 2)], topk=(1, 5))
    assert ref_out["correct"] == expect and ref_out["n"] == n

    batch = pp.pack_images(ims, "cuda")
    logits = []

    def tf(rag):
        q = pp.eval_transform_pil(rag, s_in, size, crop)
        logits.append(eng.forward(q).cpu().numpy().copy())
        return q
    out = evaluate(eng, [(batch[a:a + 2], labels[a:a + 2]) for a in range(0, n, 2)], topk=(1, 5), transform=tf)
    assert out == ref_out
    assert np.array_equal(np.concatenate(logits), logits_ref)
