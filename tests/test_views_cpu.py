"""Image views without a GPU: include/ivit_views.h declares three entries under version 1 beside nine unchanged headers, the binding
follows it and the build its mtime; `views_reference` equals every recorded view of tests/golden/pil_views.npz (written by Pillow)
and LIVE Pillow on seeded random cases; the builders (centre, five-crop, ten-crop, boxes, random resized crops) against Pillow applied
by hand; `view_sum_reference`; the fixture holds every class its tool promises."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import ivit_amd as iv
from ivit_amd import _abi, _lib
from ivit_amd import preprocess as pp
from ivit_amd import views as vw
from ivit_amd.predict import view_scale_reference, view_sum_reference
from pil_views_fixture import group_ids, views_fixture
from test_search_cpu import _prototypes_digest

ENTRIES = {"ivit_view_resize_u8_pil": 11, "ivit_view_transform_u8": 14, "ivit_logits_view_sum": 6}


# ---------------------------------------------------------------- the tenth header and its binding
def test_views_header_declares_entries_and_version():
    hdr = open(os.path.join(ROOT, "include", "ivit_views.h")).read()
    assert re.search(r'#include "ivit\.h"', hdr)
    assert int(re.search(r"#define IVIT_VIEWS_VERSION (\d+)", hdr).group(1)) == 1 == _lib.IVIT_VIEWS_VERSION
    assert _abi.VIEWS_ABI.constants == {"IVIT_VIEWS_VERSION": 1}
    assert list(_abi.VIEWS_ABI.functions) == list(ENTRIES)
    for name in ENTRIES:                                  # one "Alignment:" and one "Overlap:" line in front of every entry
        m = re.search(r"\bint %s\(" % name, hdr)
        front = hdr[hdr.rfind(";", 0, m.start()) + 1:m.start()]
        assert len(re.findall(r"\bAlignment:", front)) == 1 and len(re.findall(r"\bOverlap:", front)) == 1, name
    assert [d.name for d in _abi.VIEWS_ABI.structs["ivit_view_desc"]] == list(vw.VIEW_FIELDS)
    assert all(d.base == "int32_t" and not d.ptr and not d.array for d in _abi.VIEWS_ABI.structs["ivit_view_desc"])
    assert [p.name for p in _abi.VIEWS_ABI.functions["ivit_view_resize_u8_pil"].params] == [
        "h", "pixels", "pixels_bytes", "img_host", "img_dev", "B", "view_host", "view_dev", "V", "crop", "out_hwc"]
    assert [p.name for p in _abi.VIEWS_ABI.functions["ivit_view_transform_u8"].params] == [
        "h", "pixels", "pixels_bytes", "img_host", "img_dev", "B", "view_host", "view_dev", "V", "crop", "mean_host", "std_host", "scale", "nchw"]
    assert [p.name for p in _abi.VIEWS_ABI.functions["ivit_logits_view_sum"].params] == ["h", "logits", "groups", "views", "num_classes", "out"]


# the nine older headers: prototype count, version and sha256 of their prototypes (names, parameter types and names, in order).  The
# first eight are those test_probe_cpu.py pins; ivit_probe.h's was computed with the same function on the parent commit
OLDER_HEADERS = {"ivit.h": (99, 111, "6817c4e822691347e82f51942395393d315550b28b44df8fd32f8d739abd6b52"),
                 "ivit_eval.h": (5, 1, "b47eee22a4d967fa3efca30b6994987eecccbe61cf040a3608941660bf3bee07"),
                 "ivit_features.h": (5, 1, "cb523d76e256d935c2b277e969372ad9fbcde8cbdb97559fa7d84a6516f2159f"),
                 "ivit_attnmap.h": (4, 1, "2f429e1f49a79e9a910707d666d5d274831c1f49f0e8177fd51abf43952572f6"),
                 "ivit_classmap.h": (3, 1, "8da355354133cbf09e4e986c0bb6e4081b79ba6c60ac3fdb746cceec64bc3620"),
                 "ivit_hidden.h": (7, 1, "e32b2dd1cfd7fa95a32729c1e3b888b5f32d46680928bf55b727671ba8d2f93f"),
                 "ivit_search.h": (4, 1, "9eb19bc2c54d09c40ef4eee451c7ed84db075aa304ded29c967e5abbfc9c57cb"),
                 "ivit_modelfile.h": (9, 1, "cc004a1a3defcd124101e555c0ea3f5479b1b478141e709a622a4103294fac1c"),
                 "ivit_probe.h": (1, 1, "4eaa49a087e0d7be3debf4471f709a729ef3bed15de73d93227da2acfb557689")}


def test_views_entries_bound_and_exported_beside_unchanged_headers():
    iv.build()
    lib = _lib.load()
    P, I, Z, F = _lib._P, _lib._I, ctypes.c_size_t, ctypes.c_float
    assert list(_lib.VIEWS_SIGNATURES) == list(ENTRIES) == list(_lib.VIEWS_RESTYPES)
    for name, nparams in ENTRIES.items():             # every bound name is exported, with the header's parameter count
        bound = getattr(lib, name)
        assert len(_lib.VIEWS_SIGNATURES[name]) == nparams and bound.argtypes == _lib.VIEWS_SIGNATURES[name] and bound.restype is I, name
    assert _lib.VIEWS_SIGNATURES["ivit_view_resize_u8_pil"] == [P, P, Z, P, P, I, P, P, I, I, P]
    assert _lib.VIEWS_SIGNATURES["ivit_view_transform_u8"] == [P, P, Z, P, P, I, P, P, I, I, P, P, F, P]
    assert _lib.VIEWS_SIGNATURES["ivit_logits_view_sum"] == [P, P, I, I, I, P]
    assert ctypes.sizeof(_lib.ViewDesc) == 40 == vw.VIEW_DTYPE.itemsize
    assert [(n, ctypes.c_int32) for n in vw.VIEW_FIELDS] == [(n, t) for n, t in _lib.ViewDesc._fields_]
    assert [vw.VIEW_DTYPE.fields[n][1] for n in vw.VIEW_FIELDS] == [getattr(_lib.ViewDesc, n).offset for n in vw.VIEW_FIELDS]
    versions = (_lib.IVIT_VERSION, _lib.IVIT_EVAL_VERSION, _lib.IVIT_FEATURES_VERSION, _lib.IVIT_ATTNMAP_VERSION, _lib.IVIT_CLASSMAP_VERSION,
                _lib.IVIT_HIDDEN_VERSION, _lib.IVIT_SEARCH_VERSION, _lib.IVIT_MODELFILE_VERSION, _lib.IVIT_PROBE_VERSION)
    abis = (_lib.ABI, _lib.EVAL_ABI, _lib.FEATURES_ABI, _lib.ATTNMAP_ABI, _lib.CLASSMAP_ABI, _lib.HIDDEN_ABI, _lib.SEARCH_ABI, _lib.MODELFILE_ABI,
            _lib.PROBE_ABI)
    older = set()
    for (name, (count, version, digest)), abi, v in zip(OLDER_HEADERS.items(), abis, versions):
        assert len(abi.functions) == count and v == version and _prototypes_digest(abi) == digest, name
        text = open(os.path.join(ROOT, "include", name)).read()
        assert _prototypes_digest(_abi.parse(text) if name == "ivit.h" else _abi.parse(text, base=_lib.ABI)) == digest, name
        assert "ivit_view" not in text, name
        older |= set(abi.functions)
    assert not set(ENTRIES) & older
    with pytest.raises(_abi.AbiError):                    # it names a handle of ivit.h: it parses only with ivit.h as its base
        _abi.parse(open(_abi.VIEWS_HEADER).read())


def test_build_follows_the_views_header():
    so = iv.build()
    assert os.path.getmtime(so) >= os.path.getmtime(_abi.VIEWS_HEADER)
    assert "ivit_views.h" in _lib.SOURCES and os.path.exists(os.path.join(ROOT, "i-vit_amd", "csrc", "ivit_views.h"))
    src = open(os.path.join(ROOT, "i-vit_amd", "_lib.py")).read()
    assert re.search(r"newest = max\(.*_abi\.PROBE_HEADER, _abi\.VIEWS_HEADER", src)


def test_views_on_both_engines():
    import inspect
    from ivit_amd import predict
    from ivit_amd.engine import ViTEngine
    from ivit_amd.native import NativeEngine
    from ivit_amd.swin_engine import SwinEngine
    for cls in (NativeEngine, ViTEngine, SwinEngine):
        assert list(inspect.signature(cls.predict_views).parameters)[1:4] == ["images", "views", "k"], cls
        assert list(inspect.signature(cls.score_views).parameters)[1:4] == ["images", "labels", "views"], cls
    par = inspect.signature(predict.evaluate).parameters
    assert list(par)[:7] == ["engine", "batches", "topk", "transform", "rank", "world", "loss"] and par["views"].default == 1


def test_evaluate_refuses_views_outside_1_to_64_before_it_reads_a_batch():
    from ivit_amd.predict import evaluate

    def batches():
        raise AssertionError("a batch was asked for")
        yield
    for bad in (0, 65, -1):
        for loss in (False, True):
            with pytest.raises(ValueError, match="views"):
                evaluate(None, batches(), views=bad, loss=loss)


# ---------------------------------------------------------------- the numpy statement against Pillow
@pytest.mark.parametrize("k", range(len(group_ids())), ids=group_ids())
def test_reference_equals_every_recorded_view(k):
    _, images, groups = views_fixture()
    crop, views, want = groups[k]
    got = vw.views_reference(images, views, crop)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), [int((a != b).sum()) for a, b in zip(got, want)]


def _pil_view(im, v, crop):
    from PIL import Image
    x0, y0, bw, bh, rw, rh, left, top = (int(v[n]) for n in vw.VIEW_FIELDS[1:9])
    out = Image.fromarray(im, "RGB").crop((x0, y0, x0 + bw, y0 + bh)).resize((rw, rh), Image.BICUBIC).crop((left, top, left + crop, top + crop))
    return np.asarray(out.transpose(Image.FLIP_LEFT_RIGHT) if v["flip"] else out)


def test_reference_equals_live_pillow_on_random_cases():
    """60 seeded cases: a box inside a larger image, a random resized size and window; every sixth case copies the horizontal axis,
    every seventh the vertical one, every fifth is a down-scale above 23.5 (the vertical taps of the device's streaming form)"""
    pytest.importorskip("PIL")
    rng = np.random.Generator(np.random.PCG64(2024))
    copied, steep = 0, 0
    for case in range(60):
        crop = (1, 7, 16, 33)[case % 4]
        H, W = int(rng.integers(100, 131)), int(rng.integers(100, 131))
        im = rng.integers(0, 256, (H, W, 3), dtype=np.uint8) if case % 3 else (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
        if case % 5 == 0:                                 # a down-scale above 23.5: only a crop of 1 .. 3 fits
            crop = 1
            bw, bh = int(rng.integers(48, 91)), int(rng.integers(48, 91))
            rw, rh = int(rng.integers(1, 3)), int(rng.integers(1, 3))
            if case % 10 == 0:
                bw, rw = 90, 1                            # the largest: 90
        else:
            bw, bh = int(rng.integers(1, 91)), int(rng.integers(1, 91))
            rw, rh = int(rng.integers(crop, crop + 40)), int(rng.integers(crop, crop + 40))
            if case % 6 == 1 and bw >= crop:
                rw = bw
            if case % 7 == 2 and bh >= crop:
                rh = bh
        x0, y0 = int(rng.integers(1, W - bw)), int(rng.integers(1, H - bh))
        left, top = int(rng.integers(0, rw - crop + 1)), int(rng.integers(0, rh - crop + 1))
        views = vw.make_views([(0, x0, y0, bw, bh, rw, rh, left, top, case % 2)])
        copied += (rw == bw) + (rh == bh)
        steep += max(bw / rw, bh / rh) > 23.5
        got = vw.views_reference([im], views, crop)[0]
        want = _pil_view(im, views[0], crop)
        assert np.array_equal(got, want), (case, views[0], crop, int((got != want).sum()))
    assert copied >= 6 and steep >= 10


def _sample_images():
    rng = np.random.Generator(np.random.PCG64(77))
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((41, 58), (63, 40), (36, 36))]


def test_center_views_are_the_eval_transform():
    ims = _sample_images()
    for size, crop in ((36, 32), (30, 30), (50, 33)):
        views = vw.center_views(pp.pack_images(ims, "cpu"), size, crop)
        assert len(views) == len(ims) and views["image"].tolist() == [0, 1, 2] and not views["flip"].any()
        assert np.array_equal(vw.views_reference(ims, views, crop), pp.pil_resize_center_crop_reference(ims, size, crop))
    with pytest.raises(ValueError, match="image 0: crop"):
        vw.center_views(ims, 20, 21)


def test_five_and_ten_crop_views_are_pillows_crops_of_the_resized_image_and_of_its_mirror_image():
    """non-square images; 41 x 58 at size 37 -> 37 x 52, crop 32: both (dim - crop) odd (5 and 20 ... the second image gives the
    odd width), so the centre of the mirror image is NOT the mirrored centre"""
    Image = pytest.importorskip("PIL.Image")
    ims = _sample_images()
    size, crop = 37, 32
    five, ten = vw.five_crop_views(ims, size, crop), vw.ten_crop_views(ims, size, crop)
    assert len(five) == 15 and len(ten) == 30
    assert five["image"].tolist() == [i for i in range(3) for _ in range(5)] and ten["image"].tolist() == [i for i in range(3) for _ in range(10)]
    got5, got10 = vw.views_reference(ims, five, crop), vw.views_reference(ims, ten, crop)
    odd = 0
    for i, im in enumerate(ims):
        Hr, Wr = pp.resized_size(im.shape[0], im.shape[1], size)
        odd += (Wr - crop) % 2
        resized = Image.fromarray(im, "RGB").resize((Wr, Hr), Image.BICUBIC)
        cl, ct = pp.crop_offset(Wr, crop), pp.crop_offset(Hr, crop)
        wins = ((0, 0), (Wr - crop, 0), (0, Hr - crop), (Wr - crop, Hr - crop), (cl, ct))
        for j, pic in enumerate((resized, resized.transpose(Image.FLIP_LEFT_RIGHT))):
            for k, (x, y) in enumerate(wins):
                want = np.asarray(pic.crop((x, y, x + crop, y + crop)))
                assert np.array_equal(got10[10 * i + 5 * j + k], want), (i, j, k)
                if j == 0:
                    assert np.array_equal(got5[5 * i + k], want), (i, k)
        assert ten["flip"][10 * i:10 * i + 10].tolist() == [0] * 5 + [1] * 5
        # the mirrored five are the flipped views of top-right, top-left, bottom-right, bottom-left, and the centre of the mirror image
        assert ten["left"][10 * i + 5:10 * i + 10].tolist() == [Wr - crop, 0, Wr - crop, 0, Wr - crop - cl]
    assert odd >= 1


def test_box_views_in_both_modes():
    Image = pytest.importorskip("PIL.Image")
    ims = _sample_images()
    boxes = [(3, 5, 20, 30), (0, 0, 40, 63), (11, 2, 7, 7)]
    st = vw.box_views(1, boxes, 12)
    assert st["image"].tolist() == [1, 1, 1] and st["rw"].tolist() == st["rh"].tolist() == [12, 12, 12]
    assert not st["left"].any() and not st["top"].any() and not st["flip"].any()
    assert [tuple(int(v[n]) for n in ("x0", "y0", "bw", "bh")) for v in st] == boxes
    got = vw.views_reference(ims, st, 12)
    for j, (x0, y0, bw, bh) in enumerate(boxes):
        want = np.asarray(Image.fromarray(ims[1], "RGB").crop((x0, y0, x0 + bw, y0 + bh)).resize((12, 12), Image.BICUBIC))
        assert np.array_equal(got[j], want), j
    sh = vw.box_views(1, boxes, 6, mode="short", size=7, flip=True)
    got = vw.views_reference(ims, sh, 6)
    for j, (x0, y0, bw, bh) in enumerate(boxes):               # the eval rule on the box as an image of its own, then mirrored
        want = pp.pil_resize_center_crop_reference([ims[1][y0:y0 + bh, x0:x0 + bw]], 7, 6)[0][:, ::-1]
        assert np.array_equal(got[j], want), j
        assert (int(sh["rh"][j]), int(sh["rw"][j])) == pp.resized_size(bh, bw, 7) and sh["flip"][j] == 1
    assert vw.box_views(0, boxes[:1], 6, mode="short")["rw"][0] == 6        # size defaults to crop
    with pytest.raises(ValueError):
        vw.box_views(0, boxes, 6, mode="fit")
    with pytest.raises(ValueError, match="box 0"):
        vw.box_views(0, [(0, 0, 0, 4)], 6)


def test_random_resized_crop_views_properties():
    sides = [(41, 58), (63, 40), (36, 36), (200, 3), (2, 150)]
    views = vw.random_resized_crop_views(sides, 16, np.random.default_rng(5), per_image=40)
    assert len(views) == 200 and views["image"].tolist() == [i for i in range(5) for _ in range(40)]
    for v in views:                                           # every box inside its image, stretched to the crop
        h, w = sides[int(v["image"])]
        assert v["bw"] >= 1 and v["bh"] >= 1 and v["x0"] >= 0 and v["y0"] >= 0 and v["x0"] + v["bw"] <= w and v["y0"] + v["bh"] <= h
        assert (v["rw"], v["rh"], v["left"], v["top"]) == (16, 16, 0, 0) and v["flip"] in (0, 1)
    vw.check_views(sides, views, 16)
    assert 0 < views["flip"].sum() < 200                      # the flip share lies strictly between 0 and 1 over 200 draws
    again = vw.random_resized_crop_views(sides, 16, np.random.default_rng(5), per_image=40)
    assert np.array_equal(views, again)                       # the same seed gives the same table
    other = vw.random_resized_crop_views(sides, 16, np.random.default_rng(6), per_image=40)
    assert not np.array_equal(views, other)
    # 200 x 3 and 2 x 150 cannot hold a box of an allowed ratio and 8 % of the area on most tries: the central fallback keeps the ratio's bound
    thin = views[views["image"] == 3]
    assert (thin["bw"] <= 3).all() and (thin["bh"] <= 200).all()
    assert not vw.random_resized_crop_views(sides, 16, np.random.default_rng(5), flip_p=0.0)["flip"].any()
    assert vw.random_resized_crop_views(sides, 16, np.random.default_rng(5), flip_p=1.0)["flip"].all()


def test_views_reference_refuses_what_the_entries_refuse():
    ims = _sample_images()
    good = (0, 3, 4, 20, 21, 10, 11, 1, 2, 0)
    assert vw.views_reference(ims, vw.make_views([good]), 8).shape == (1, 8, 8, 3)
    for pos, value, word in ((0, 3, "image"), (0, -1, "image"), (3, 56, "box"), (4, 38, "box"), (3, 0, "box"), (1, -1, "box"), (5, 0, "resized"),
                             (5, 65537, "resized"), (7, 3, "window"), (8, 4, "window"), (7, -1, "window"), (9, 2, "flip")):
        row = list(good)
        row[pos] = value
        with pytest.raises(ValueError, match=f"view 1: {word}"):
            vw.views_reference(ims, vw.make_views([good, row]), 8)


# ---------------------------------------------------------------- the sum of the views' logits
def test_view_sum_reference():
    acc = np.array([[1, -2, 2147483647, -2147483648, 5],
                    [3, -4, 1, -1, 6],
                    [7, 8, 2147483647, -2147483648, -11],
                    [0, 0, 0, 0, 0]], np.int32)
    got = view_sum_reference(acc, 2)
    assert got.dtype == np.int32 and got.tolist() == [[4, -6, 2147483647, -2147483648, 11], [7, 8, 2147483647, -2147483648, -11]]
    assert view_sum_reference(acc, 4).tolist() == [[11, 2, 2147483647, -2147483648, 0]]      # 2^32 - 1 and -2^32 - 1: both ends saturate
    one = view_sum_reference(acc, 1)
    assert one.dtype == np.int32 and np.array_equal(one, acc)                                # views = 1 is the identity
    assert view_sum_reference(np.zeros((0, 5), np.int32), 3).shape == (0, 5)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="views"):
            view_sum_reference(acc, bad)
    with pytest.raises(ValueError, match="multiple"):
        view_sum_reference(acc, 3)
    s = np.array([0.5, 3.0, 1e-3], np.float32)
    v = view_scale_reference(s, 10)
    assert v.dtype == np.float32 and np.array_equal(v, s / np.float32(10.0)) and np.array_equal(view_scale_reference(s, 1), s)


# ---------------------------------------------------------------- what the fixture holds
def test_fixture_holds_every_class():
    g, images, groups = views_fixture()
    assert len(g["bytes"]) == int((g["crops"].astype(np.int64) ** 2 * 3).sum()) and g["views"].shape == (len(g["crops"]), 10)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "pil_views.npz")) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "pil_resize.npz"))
    allv = [(v, crop) for crop, views, _ in groups for v in views]
    for crop, views, _ in groups:
        vw.check_views([im.shape[:2] for im in images], views, crop)
    sides = {j: images[j].shape[:2] for j in range(len(images))}

    def some(pred):
        return any(pred(v, c, *sides[int(v["image"])]) for v, c in allv)
    assert some(lambda v, c, h, w: v["rw"] > v["bw"]) and some(lambda v, c, h, w: v["rw"] < v["bw"])          # up and down, horizontally
    assert some(lambda v, c, h, w: v["rh"] > v["bh"]) and some(lambda v, c, h, w: v["rh"] < v["bh"])          # and vertically
    assert some(lambda v, c, h, w: v["rw"] > v["bw"] and v["rh"] < v["bh"]) and some(lambda v, c, h, w: v["rw"] < v["bw"] and v["rh"] > v["bh"])
    assert some(lambda v, c, h, w: v["rw"] == v["bw"] and v["rh"] != v["bh"]) and some(lambda v, c, h, w: v["rh"] == v["bh"] and v["rw"] != v["bw"])
    assert some(lambda v, c, h, w: v["rw"] == v["bw"] and v["rh"] == v["bh"])
    assert some(lambda v, c, h, w: v["bw"] == 1 and v["bh"] > 1 and w > 1) and some(lambda v, c, h, w: v["bh"] == 1 and v["bw"] > 1)
    assert some(lambda v, c, h, w: v["x0"] == 0 and v["bw"] < w) and some(lambda v, c, h, w: v["y0"] == 0 and v["bh"] < h)
    assert some(lambda v, c, h, w: v["x0"] + v["bw"] == w and v["x0"] > 0) and some(lambda v, c, h, w: v["y0"] + v["bh"] == h and v["y0"] > 0)
    assert some(lambda v, c, h, w: (v["x0"], v["y0"], v["bw"], v["bh"]) == (0, 0, w, h))
    assert some(lambda v, c, h, w: 0 < v["x0"] and v["x0"] + v["bw"] < w and 0 < v["y0"] and v["y0"] + v["bh"] < h)      # strictly inside
    for cx, cy in ((0, 0), (1, 0), (0, 1), (1, 1)):           # windows at all four corners of a resized box larger than the crop
        assert some(lambda v, c, h, w: v["rw"] > c and v["rh"] > c and v["left"] == cx * (v["rw"] - c) and v["top"] == cy * (v["rh"] - c)), (cx, cy)
    assert some(lambda v, c, h, w: v["flip"] == 1 and c % 2 == 1 and c > 1) and some(lambda v, c, h, w: v["flip"] == 1 and c % 2 == 0)
    assert some(lambda v, c, h, w: c == 1)
    assert some(lambda v, c, h, w: set(np.unique(images[int(v["image"])])) <= {0, 255})                    # a saturated image
    # the ten-crop of one image: the table ten_crop_views gives, bytes taken by hand from the resized image and its mirror image
    image, size, crop, first = (int(t) for t in g["tencrop"])
    table = vw.ten_crop_views([images[image].shape[:2]], size, crop)
    table["image"] = image
    assert np.array_equal(vw.make_views(g["views"][first:first + 10]), table) and (g["crops"][first:first + 10] == crop).all()
    Hr, Wr = pp.resized_size(*images[image].shape[:2], size)
    assert (Hr - crop) % 2 == 1 and (Wr - crop) % 2 == 1
