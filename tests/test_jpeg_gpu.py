"""JPEG input on the device (include/ivit_jpeg.h): ivit_jpeg_reconstruct_u8 against Pillow's recorded bytes (tests/golden/jpeg.npz:
every byte, no tolerance) in one ragged call, one image per call and in reversed order; the decoded pool through the eval transform and
both micro engines against the same on Pillow's bytes; guards, unchanged inputs, the alignment, overlap and range refusals; a captured
reconstruction replayed over other coefficients; `jpeg.decode` with its fallbacks; examples/classify_jpeg.c against Python."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden, golden_scales

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from ivit_amd import jpeg as J  # noqa: E402
from ivit_amd import preprocess as pp  # noqa: E402

GUARD = 4096                 # bytes around every device array
FILL = 0xA5


def P(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(None)
def golden():
    z = load_golden("jpeg.npz")
    return {k: z[k] for k in z.files}


def accepted():
    return [str(n) for n in golden()["accepted"]]


@functools.lru_cache(None)
def host(name):
    """(descriptor, coefficient count, plane bytes, coefficients) of a fixture, decoded once by the library's host entries"""
    data = golden()["jpg_" + name].tobytes()
    desc, n, nws = J.query(data)
    _, coefs = J.entropy_decode(data)
    return desc, n, nws, coefs


class Placed:
    """a batch in guarded device arrays: `gap` bytes (filled) between the images' pixels, between their planes, and 8 * gap elements
    between their coefficients"""
    def __init__(self, names, gap=0):
        self.names, self.B = names, len(names)
        hs = [host(n) for n in names]
        self.table, nc, npx, nws = J.layout([x[0] for x in hs], [x[1] for x in hs], [x[2] for x in hs])
        for i in range(self.B):                                       # spread the files apart
            self.table[i].coef_offset += 8 * gap * i
            self.table[i].pixel_offset += gap * i
            self.table[i].plane_offset += 16 * gap * i
        self.nc, self.npx, self.nws = nc + 8 * gap * self.B, npx + gap * self.B, nws + 16 * gap * self.B
        coefs = np.full(self.nc + GUARD, 0x5A5A, np.int16)
        for i, x in enumerate(hs):
            a = GUARD // 2 + self.table[i].coef_offset
            coefs[a:a + x[1]] = x[3]
        self.coefs_host = coefs
        self.coefs = torch.from_numpy(coefs).cuda()
        self.pixels = torch.full((self.npx + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.work = torch.full((self.nws + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
        raw = np.frombuffer(self.table, np.uint8, self.B * ctypes.sizeof(_lib.JpegDesc)).copy()
        self.table_host = raw
        self.table_dev = torch.from_numpy(np.concatenate([np.full(GUARD, FILL, np.uint8), raw, np.full(GUARD, FILL, np.uint8)])).cuda()

    def args(self):
        return [P(self.coefs, GUARD), ctypes.c_int64(self.nc), ctypes.cast(self.table, ctypes.c_void_p), P(self.table_dev, GUARD), self.B,
                P(self.work, GUARD), ctypes.c_size_t(self.nws), P(self.pixels, GUARD), ctypes.c_size_t(self.npx)]

    def run(self, H):
        H.call("ivit_jpeg_reconstruct_u8", *self.args())
        torch.cuda.synchronize()
        return self.check()

    def check(self, written=True):
        """guards, gaps and inputs; -> the images"""
        px, wk = self.pixels.cpu().numpy(), self.work.cpu().numpy()
        assert (px[:GUARD] == FILL).all() and (px[GUARD + self.npx:] == FILL).all(), "wrote outside pixels"
        assert (wk[:GUARD] == FILL).all() and (wk[GUARD + self.nws:] == FILL).all(), "wrote outside the workspace"
        assert np.array_equal(self.coefs.cpu().numpy(), self.coefs_host), "coefficients changed"
        td = self.table_dev.cpu().numpy()
        assert (td[:GUARD] == FILL).all() and (td[GUARD + len(self.table_host):] == FILL).all() and np.array_equal(
            td[GUARD:GUARD + len(self.table_host)], self.table_host), "device table changed"
        assert np.array_equal(np.frombuffer(self.table, np.uint8, len(self.table_host)), self.table_host), "host table changed"
        if not written:
            assert (px == FILL).all() and (wk == FILL).all(), "a refused call wrote"
            return None
        out, covered_px, covered_wk = [], np.zeros(self.npx, bool), np.zeros(self.nws, bool)
        for i in range(self.B):
            d = self.table[i]
            n = d.w * d.h * 3
            out.append(px[GUARD + d.pixel_offset:GUARD + d.pixel_offset + n].reshape(d.h, d.w, 3))
            covered_px[d.pixel_offset:d.pixel_offset + n] = True
            covered_wk[d.plane_offset:d.plane_offset + host(self.names[i])[2]] = True
        assert (px[GUARD:GUARD + self.npx][~covered_px] == FILL).all(), "wrote between the images"
        assert (wk[GUARD:GUARD + self.nws][~covered_wk] == FILL).all(), "wrote between the planes"
        return out


def _assert_pil(names, images):
    g = golden()
    for n, im in zip(names, images):
        want = g["rgb_" + n]
        assert im.shape == want.shape and np.array_equal(im, want), (n, int((im != want).sum()))


# ---------------------------------------------------------------- decoding
def test_all_fixtures_in_one_ragged_call_equal_pil_bytes(H):
    names = accepted()
    _assert_pil(names, Placed(names, gap=5).run(H))


def test_reversed_batch_equals_pil_bytes(H):
    names = accepted()[::-1]
    _assert_pil(names, Placed(names, gap=3).run(H))


def test_one_image_per_call_equals_pil_bytes(H):
    """one shared set of buffers, one call per file (the buffers are large enough for the largest)"""
    names = accepted()
    g = golden()
    nc, nws, npx = max(host(n)[1] for n in names), max(host(n)[2] for n in names), max(g["rgb_" + n].size for n in names)
    coefs = torch.zeros(nc, dtype=torch.int16, device="cuda")
    work = torch.zeros(nws + 64, dtype=torch.uint8, device="cuda")
    pixels = torch.zeros(npx + 64, dtype=torch.uint8, device="cuda")
    for n in names:
        desc, k, w, c = host(n)
        coefs[:k] = torch.from_numpy(c).cuda()
        table, _, _, _ = J.layout([desc], [k], [w])
        pixels.fill_(FILL)
        J.reconstruct(coefs, table, 1, pixels, work, h=H)
        got = pixels.cpu().numpy()
        want = g["rgb_" + n]
        assert np.array_equal(got[:want.size].reshape(want.shape), want) and (got[want.size:] == FILL).all(), n


def test_empty_batch_launches_nothing(H):
    p = Placed(accepted()[:3])
    a = p.args()
    a[4] = 0
    H.call("ivit_jpeg_reconstruct_u8", *a)
    H.call("ivit_jpeg_reconstruct_u8", None, ctypes.c_int64(0), None, None, 0, None, ctypes.c_size_t(0), None, ctypes.c_size_t(0))
    torch.cuda.synchronize()
    p.check(written=False)
    n = ctypes.c_size_t(7)
    assert H.lib.ivit_jpeg_workspace_bytes(None, 0, ctypes.byref(n)) == _lib.IVIT_OK and n.value == 0
    assert H.lib.ivit_jpeg_workspace_bytes(ctypes.cast(p.table, ctypes.c_void_p), 3, ctypes.byref(n)) == _lib.IVIT_OK and n.value == p.nws


# ---------------------------------------------------------------- chaining
def test_eval_transform_on_the_decoded_pool_equals_the_same_on_pil_bytes():
    g, names = golden(), accepted()
    batch, fallbacks = J.decode([g["jpg_" + n].tobytes() for n in names], "cuda", threads=4)
    assert fallbacks == [] and len(batch) == len(names)
    ref = pp.pack_images([g["rgb_" + n] for n in names], "cuda")
    assert np.array_equal(batch.desc, ref.desc) and torch.equal(batch.pixels, ref.pixels)
    for size, crop in ((20, 16), (9, 7)):
        assert torch.equal(pp.eval_transform_pil(batch, 0.03, size, crop), pp.eval_transform_pil(ref, 0.03, size, crop))
        assert torch.equal(pp.resize_center_crop_pil(batch, size, crop), pp.resize_center_crop_pil(ref, size, crop))


def _engine(fname):
    g = load_golden(fname)
    if str(g["cfg_name"]) in iv.SWIN_CONFIGS:
        from ivit_amd.swin_engine import SwinEngine
        cfg = iv.SWIN_CONFIGS[str(g["cfg_name"])]
        return cfg, SwinEngine(cfg, iv.make_swin_weights(cfg, int(g["seed"])), golden_scales(g))
    from ivit_amd.engine import ViTEngine
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    return cfg, ViTEngine.from_float(cfg, iv.make_vit_weights(cfg, int(g["seed"])), golden_scales(g))


ENGINE_FILES = ["64x48_noise_q85_s2", "53x37_grad_q85_s1", "17x33_noise_q30_grey", "64x48_grad_q100_s0"]


@pytest.mark.parametrize("fname", ["micro_vit_b2.npz", "micro_swin_b2.npz"])
def test_logits_from_decode_equal_the_pil_path(fname):
    g = golden()
    cfg, eng = _engine(fname)
    crop, size, s_in = cfg.img_size, cfg.img_size + 5, eng.input_scale_host()
    batch, fallbacks = J.decode([g["jpg_" + n].tobytes() for n in ENGINE_FILES], "cuda")
    assert fallbacks == []
    ref = pp.pack_images([g["rgb_" + n] for n in ENGINE_FILES], "cuda")
    a = eng.forward(pp.eval_transform_pil(batch, s_in, size, crop), copy=True)
    b = eng.forward(pp.eval_transform_pil(ref, s_in, size, crop), copy=True)
    assert a.shape == (len(ENGINE_FILES), cfg.num_classes) and torch.equal(a, b) and a.any()


# ---------------------------------------------------------------- contract
CONTRACT = ["17x33_noise_q85_s2", "9x7_noise_q85_s1", "16x16_grad_q30_grey", "53x37_noise_q100_s0"]


def _refused(H, p, args, *words):
    st = H.lib.ivit_jpeg_reconstruct_u8(H.h, *args)
    msg = H.lib.ivit_last_error(H.h).decode()
    assert st == _lib.IVIT_ERR_INVALID, (st, msg)
    for w in words:
        assert w in msg, msg
    torch.cuda.synchronize()
    p.check(written=False)


def test_alignment_and_overlap_are_refused_with_nothing_launched(H):
    p = Placed(CONTRACT, gap=2)
    good = p.args()
    for pos, off, name in ((0, 2, "coefs"), (0, 8, "coefs"), (5, 8, "workspace"), (5, 1, "workspace"), (3, 4, "desc_dev")):
        a = list(good)
        a[pos] = ctypes.c_void_p(good[pos].value + off)
        _refused(H, p, a, name, "aligned")
    # every "Overlap:" pair: pixels and workspace against each other, against coefs and against desc_dev
    big = torch.full((1 << 20,), FILL, dtype=torch.uint8, device="cuda")
    base = (big.data_ptr() + 255) // 256 * 256
    q = Placed(CONTRACT, gap=2)
    def over(first, second):
        """the arrays named `first` and `second` inside `big`, the second starting on the first's last 16 bytes"""
        sizes = {"coefs": q.nc * 2, "workspace": q.nws, "pixels": q.npx, "desc_dev": len(q.table_host)}
        a = list(q.args())
        pos = {"coefs": 0, "desc_dev": 3, "workspace": 5, "pixels": 7}
        a[pos[first]] = ctypes.c_void_p(base)
        a[pos[second]] = ctypes.c_void_p(base + (sizes[first] - 16) // 16 * 16)
        return a
    for first, second in (("pixels", "workspace"), ("workspace", "pixels"), ("coefs", "pixels"), ("pixels", "coefs"), ("desc_dev", "pixels"),
                          ("coefs", "workspace"), ("workspace", "coefs"), ("desc_dev", "workspace"), ("workspace", "desc_dev")):
        st = H.lib.ivit_jpeg_reconstruct_u8(H.h, *over(first, second))
        msg = H.lib.ivit_last_error(H.h).decode()
        assert st == _lib.IVIT_ERR_INVALID and "overlap" in msg and first in msg and second in msg, (first, second, msg)
    torch.cuda.synchronize()
    assert (big == FILL).all().item()
    q.check(written=False)
    _assert_pil(CONTRACT, p.run(H))                       # and the plain call on the same arrays


def test_descriptor_ranges_are_refused_with_the_image_index(H):
    p = Placed(CONTRACT)                                  # back to back: the last file ends where its buffers end
    def with_field(i, field, value, *words):
        old = getattr(p.table[i], field)
        setattr(p.table[i], field, value)
        try:
            st = H.lib.ivit_jpeg_reconstruct_u8(H.h, *p.args())
            msg = H.lib.ivit_last_error(H.h).decode()
        finally:
            setattr(p.table[i], field, old)
        assert st == _lib.IVIT_ERR_INVALID and all(w in msg for w in words), (field, value, msg)
    last = p.B - 1
    with_field(last, "coef_offset", p.table[last].coef_offset + 8, "image %d:" % last, "coef_count")
    with_field(1, "coef_offset", -8, "image 1:", "coef_offset")
    with_field(1, "coef_offset", p.table[1].coef_offset + 4, "image 1:", "multiple of 8")
    with_field(last, "pixel_offset", p.table[last].pixel_offset + 3, "image %d:" % last, "pixels_bytes")
    with_field(2, "pixel_offset", -1, "image 2:", "pixel_offset")
    with_field(2, "pixel_offset", p.table[1].pixel_offset + 1, "image 2:", "earlier image")
    with_field(last, "plane_offset", p.table[last].plane_offset + 16, "image %d:" % last, "workspace_bytes")
    with_field(1, "plane_offset", p.table[1].plane_offset + 8, "image 1:", "multiple of 16")
    with_field(2, "plane_offset", p.table[1].plane_offset, "image 2:", "earlier image")
    with_field(0, "w", 0, "image 0:", "side")
    with_field(0, "w", p.table[0].w + 16, "image 0:", "block grid")
    with_field(0, "hs", 3, "image 0:", "sampling")
    with_field(2, "hs", 2, "image 2:", "sampling")          # grey with 2x1
    with_field(1, "ncomp", 2, "image 1:", "ncomp")
    with_field(3, "reserved", 1, "image 3:", "reserved")
    a = p.args()
    a[1] = ctypes.c_int64(p.nc - 1)
    _refused(H, p, a, "image %d:" % last, "coef_count")
    a = p.args()
    a[8] = ctypes.c_size_t(p.npx - 1)
    _refused(H, p, a, "image %d:" % last, "pixels_bytes")
    a = p.args()
    a[6] = ctypes.c_size_t(p.nws - 1)
    _refused(H, p, a, "image %d:" % last, "workspace_bytes")
    for pos in (0, 2, 3, 5, 7):
        a = p.args()
        a[pos] = None
        _refused(H, p, a, "bad arguments")
    a = p.args()
    a[4] = -1
    _refused(H, p, a, "bad arguments")
    _assert_pil(CONTRACT, p.run(H))


# ---------------------------------------------------------------- capture
def test_captured_reconstruction_replays_over_other_coefficients():
    """two files of one geometry and one set of tables: the graph is captured over the first, replayed after the second's
    coefficients were copied under the same descriptors"""
    names = ["53x37_noise_q85_s2", "rst1_s2"]                # both 53 x 37, 4:2:0, quality 85
    g = golden()
    (d0, n0, w0, c0), (d1, n1, w1, c1) = host(names[0]), host(names[1])
    assert bytes(d0) == bytes(d1) and n0 == n1 and not np.array_equal(c0, c1)
    stream = torch.cuda.Stream()
    h = _lib.Handle(0, stream.cuda_stream)
    table, nc, npx, nws = J.layout([d0], [n0], [w0])
    coefs = torch.from_numpy(c0).cuda()
    work = torch.zeros(nws, dtype=torch.uint8, device="cuda")
    pixels = torch.zeros(npx, dtype=torch.uint8, device="cuda")
    table_dev = torch.from_numpy(np.frombuffer(table, np.uint8, 264).copy()).cuda()
    with torch.cuda.stream(stream):                          # eager once: the code is loaded outside the capture
        J.reconstruct(coefs, table, 1, pixels, work, table_dev=table_dev, h=h)
    torch.cuda.synchronize()
    pixels.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
        J.reconstruct(coefs, table, 1, pixels, work, table_dev=table_dev, h=h)
    torch.cuda.synchronize()
    assert not pixels.any().item()                           # captured, not run
    for n, c in ((names[0], c0), (names[1], c1), (names[0], c0)):
        coefs.copy_(torch.from_numpy(c).cuda())
        pixels.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(pixels.cpu().numpy().reshape(37, 53, 3), g["rgb_" + n]), n


# ---------------------------------------------------------------- decode
def test_decode_reports_fallbacks_and_raises_without_one(tmp_path):
    g = golden()
    pytest.importorskip("PIL")
    names = ["16x16_noise_q85_s2", "progressive", "7x9_grad_q30_grey", "cmyk", "dqt255", "1x1_noise_q85_s0"]
    datas = [g["jpg_" + n].tobytes() for n in names]
    path = tmp_path / "a.jpg"
    path.write_bytes(datas[0])
    batch, fallbacks = J.decode([str(path)] + datas[1:], "cuda", threads=3)
    assert [i for i, _ in fallbacks] == [1, 3, 4]
    assert "progressive" in fallbacks[0][1] and "4 components" in fallbacks[1][1] and "bound" in fallbacks[2][1]
    import io
    from PIL import Image
    px = batch.pixels.cpu().numpy()
    for i, d in enumerate(datas):
        want = np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))
        o = int(batch.desc["offset"][i])
        assert (batch.desc["h"][i], batch.desc["w"][i]) == want.shape[:2]
        assert np.array_equal(px[o:o + want.size].reshape(want.shape), want), names[i]
    for i in (0, 2, 5):
        assert np.array_equal(px[int(batch.desc["offset"][i]):][:g["rgb_" + names[i]].size], g["rgb_" + names[i]].reshape(-1))
    with pytest.raises(J.JpegRefused) as e:
        J.decode(datas, "cuda", fallback="raise")
    assert e.value.status == _lib.IVIT_ERR_UNSUPPORTED and "progressive" in str(e.value)
    with pytest.raises(J.JpegRefused) as e:
        J.decode([datas[0], g["jpg_trunc_20"].tobytes()], "cuda", fallback="raise")
    assert e.value.status == _lib.IVIT_ERR_INVALID


# ---------------------------------------------------------------- the C example
def test_classify_jpeg_example_gives_pythons_top_k(tmp_path):
    exe = os.path.join(ROOT, "i-vit_amd", "csrc", "classify_jpeg")
    assert os.path.exists(exe), "examples/classify_jpeg.c was not built (build() of __graft_entry__.py builds it)"
    import ivit_amd.model_file as mf
    model = os.path.join(GOLDEN, "micro_vit_b2.ivit")
    data = golden()["jpg_64x48_noise_q85_s2"].tobytes()
    path = tmp_path / "x.jpg"
    path.write_bytes(data)
    eng = mf.load_engine(model, device="cuda:0")
    cfg = eng.cfg
    k = min(3, cfg.num_classes)
    batch, _ = J.decode([data], "cuda")
    q = pp.eval_transform_pil(batch, eng.input_scale_host(), int(cfg.img_size / 0.875), cfg.img_size)
    idx, val = eng.predict(q, k=k)[:2]
    run = subprocess.run([exe, model, str(path), str(k)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    fields = run.stdout.split()
    assert fields[0] == "0" and len(fields) == 1 + k
    got_idx = [int(f.split(":")[0]) for f in fields[1:]]
    got_val = np.array([float(f.split(":")[1]) for f in fields[1:]], np.float32)
    assert got_idx == idx.cpu().numpy().reshape(-1).tolist()
    assert np.array_equal(got_val.view(np.uint32), val.cpu().numpy().reshape(-1).astype(np.float32).view(np.uint32))
    bad = tmp_path / "p.jpg"
    bad.write_bytes(golden()["jpg_progressive"].tobytes())
    run = subprocess.run([exe, model, str(bad)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 1 and "progressive" in run.stderr
