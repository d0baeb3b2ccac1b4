"""The PIL-exact ragged front end without a device: the numpy statement of its contract against PIL's recorded bytes (and live PIL
where it imports), the fixture's own guard, and the C-ABI surface (include/ivit.h, the library's exports, the binding)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import ivit_amd as iv
from ivit_amd import _lib
from ivit_amd import preprocess as pp
from pil_fixture import case_ids, fixture

NEW = ("ivit_resize_center_crop_u8_pil", "ivit_eval_transform_u8")
BAND, TILE_ROWS = 32, 96             # PIL_BAND, PIL_TILE_ROWS of csrc/ivit_preprocess.h


@pytest.mark.parametrize("k", range(len(case_ids())), ids=case_ids())
def test_reference_equals_recorded_pil_bytes(k):
    _, images, cases = fixture()
    size, crop, idx, want = cases[k]
    got = pp.pil_resize_center_crop_reference([images[i] for i in idx], size, crop)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), [int((a != b).sum()) for a, b in zip(got, want)]


def test_reference_equals_live_pil_on_random_shapes():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.Generator(np.random.PCG64(7))
    for n in range(40):
        h, w, size = int(rng.integers(1, 151)), int(rng.integers(1, 151)), int(rng.integers(1, 97))
        im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if n % 3 else (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
        Hr, Wr = pp.resized_size(h, w, size)
        crop = int(rng.integers(1, min(Hr, Wr, 64) + 1))
        top, left = pp.crop_offset(Hr, crop), pp.crop_offset(Wr, crop)
        want = np.asarray(Image.fromarray(im, "RGB").resize((Wr, Hr), Image.BICUBIC).crop((left, top, left + crop, top + crop)))
        got = pp.pil_resize_center_crop_reference([im], size, crop)[0]
        assert np.array_equal(got, want), (h, w, size, crop, int((got != want).sum()))


def _ksize(n_in, n_out):
    """PIL's bound on the tap count of one axis, the quantity the kernel switches forms on (1: the axis is copied)"""
    return 1 if n_in == n_out else 2 * math.ceil(2.0 * max(n_in / n_out, 1.0)) + 1


def test_fixture_holds_every_content_class():
    """asserted from the descriptors: a regenerated fixture that loses a class fails here, not silently in the device tests"""
    g, images, cases = fixture()
    assert str(g["pillow_version"]) and int(g["seed"]) > 0
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "pil_resize.npz")) < 600 * 1024
    assert np.array_equal(g["offsets"], np.cumsum([im.size for im in images]) - [im.size for im in images])
    seen = set()
    for size, crop, idx, out in cases:
        assert out.shape == (len(idx), crop, crop, 3)
        full, part = divmod(crop, BAND)
        if full >= 2 and part:
            seen.add("two full bands and a partial one")
        if full == 0:
            seen.add("a single partial band")
        for i in idx:
            h, w = images[i].shape[:2]
            Hr, Wr = pp.resized_size(h, w, size)
            assert crop <= min(Hr, Wr)
            if Hr < h and Wr < w:
                seen.add("portrait down-scale" if h > w else "landscape down-scale")
            if Hr > h and Wr > w:
                seen.add("up-scale")
            if min(h, w) == size and h != w:          # the shorter side is `size` already: the longer keeps its length too
                assert (Hr, Wr) == (h, w)
                seen.add("short side == size, rows cropped" if h > w else "short side == size, columns cropped")
            if h == w and size == crop:
                seen.add("square with size == crop")
            for dim, name in ((Hr, "rows"), (Wr, "columns")):
                if (dim - crop) % 2:
                    seen.add(f"odd margin of {name}, half on an {'even' if ((dim - crop) // 2) % 2 == 0 else 'odd'} integer")
            if min(h, w) == 1:
                seen.add("1-pixel strip")
            kv = _ksize(h, Hr)
            if TILE_ROWS - 3 <= kv <= TILE_ROWS:
                seen.add("tiled, next to the switch")
            if TILE_ROWS < kv <= TILE_ROWS + 3:
                seen.add("streaming, next to the switch")
            vals = np.unique(images[i])
            seen.add("saturated pixels" if set(vals.tolist()) <= {0, 255} else "random pixels")
    want = {"two full bands and a partial one", "a single partial band", "portrait down-scale", "landscape down-scale", "up-scale",
            "short side == size, rows cropped", "short side == size, columns cropped", "square with size == crop", "1-pixel strip",
            "odd margin of rows, half on an even integer", "odd margin of rows, half on an odd integer",
            "odd margin of columns, half on an even integer", "odd margin of columns, half on an odd integer",
            "tiled, next to the switch", "streaming, next to the switch", "saturated pixels", "random pixels"}
    assert want <= seen, sorted(want - seen)
    # the constants this guard restates are the kernel's
    src = open(os.path.join(ROOT, "i-vit_amd", "csrc", "ivit_preprocess.h")).read()
    assert re.search(r"#define PIL_BAND %d\b" % BAND, src) and re.search(r"#define PIL_TILE_ROWS %d\b" % TILE_ROWS, src)


def test_offsets_round_half_to_even():
    assert [pp.crop_offset(d, 72) for d in (85, 87, 80, 111)] == [6, 8, 4, 20]
    assert pp.resized_size(375, 500, 256) == (256, 341) and pp.resized_size(500, 375, 256) == (341, 256)


def test_new_entries_are_declared_exported_and_bound():
    iv.build()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ivit.h")).read()
    assert re.search(r"#define IVIT_VERSION 111\b", hdr) and lib.ivit_version() == 111
    assert "typedef struct ivit_image_desc" in hdr
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]
    assert len(_lib.SIGNATURES[NEW[0]]) == 9 and len(_lib.SIGNATURES[NEW[1]]) == 12
    assert ctypes.sizeof(_lib.ImageDesc) == 16 == pp.DESC_DTYPE.itemsize
    assert [pp.DESC_DTYPE.fields[n][1] for n in ("offset", "h", "w")] == [_lib.ImageDesc.offset.offset, _lib.ImageDesc.h.offset, _lib.ImageDesc.w.offset]
    # each declaration cites the reference's transform and names its pin
    for name in NEW:
        at = hdr.index("int " + name)
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert "utils/data_utils.py:82-92" in comment and "tests/golden/pil_resize.npz" in comment, name
