"""Image views (include/ivit_views.h): a box of an image, resized as PIL resizes a stand-alone image, a crop x crop window of that,
optionally mirrored left-right — `Image.crop(box).resize((rw, rh), BICUBIC).crop(window)[.transpose(FLIP_LEFT_RIGHT)]` — for any
number of views of the images of a `preprocess.RaggedImages` in ONE launch.

  * a view table is a numpy array of VIEW_DTYPE (struct ivit_view_desc), image-major where a builder makes it;
  * the builders are host-only: `center_views` (the eval transform's view), `five_crop_views` / `ten_crop_views` (the usual
    companions of validate(): Pillow's crops of the resized image and of its mirror image are the definition),
    `box_views` (regions: a detector's boxes, tiles of a scan) and `random_resized_crop_views` (augmented views for a probe: the
    project's own statement of the usual algorithm, pinned to nothing outside);
  * `view_resize` (uint8 HWC) and `view_transform` (int8 NCHW, what the engines read) are the device calls, one launch each;
  * `views_reference` is the numpy statement, built on `preprocess._pil_pass`; tests/golden/pil_views.npz (written by Pillow,
    tools/make_pil_views_fixture.py) pins both.

The views of one image go through an engine as a batch of their own; `engine.predict_views` / `engine.score_views` and
`predict.evaluate(..., views=V)` combine their logits (the integer sum: `predict.view_sum_reference`)."""
import ctypes

import numpy as np
import torch

from . import _lib
from . import preprocess as pp
from .quant_modules import handle

VIEW_FIELDS = ("image", "x0", "y0", "bw", "bh", "rw", "rh", "left", "top", "flip")
VIEW_DTYPE = np.dtype([(n, "<i4") for n in VIEW_FIELDS])                  # struct ivit_view_desc, 40 bytes
assert VIEW_DTYPE.itemsize == ctypes.sizeof(_lib.ViewDesc) == 40


def _sides(batch):
    """[(h, w)] of a RaggedImages, of its descriptor table or of a list of (h, w) pairs / images"""
    desc = getattr(batch, "desc", batch)
    if isinstance(desc, np.ndarray) and desc.dtype == pp.DESC_DTYPE:
        return [(int(d["h"]), int(d["w"])) for d in desc]
    return [tuple(int(v) for v in (np.shape(im)[:2] if np.ndim(im) == 3 else im)) for im in desc]


def make_views(rows):
    """rows of ten integers in the order of VIEW_FIELDS -> view table"""
    out = np.zeros(len(rows), VIEW_DTYPE)
    for i, row in enumerate(rows):
        out[i] = tuple(int(v) for v in row)
    return out


def _resized(i, h, w, size, crop):
    Hr, Wr = pp.resized_size(h, w, size)
    if crop > Hr or crop > Wr:
        raise ValueError(f"image {i}: crop {crop} larger than the resized image {Hr} x {Wr}")
    return Hr, Wr


def center_views(batch, size, crop):
    """the eval transform's view of every image: the whole image, torchvision's Resize(size) and CenterCrop(crop) geometry
    (`preprocess.resized_size`, `preprocess.crop_offset`); one view per image"""
    rows = []
    for i, (h, w) in enumerate(_sides(batch)):
        Hr, Wr = _resized(i, h, w, size, crop)
        rows.append((i, 0, 0, w, h, Wr, Hr, pp.crop_offset(Wr, crop), pp.crop_offset(Hr, crop), 0))
    return make_views(rows)


def _five(i, h, w, Hr, Wr, crop, mirrored):
    """top-left, top-right, bottom-left, bottom-right, centre of the resized image — or, `mirrored`, of its mirror image: the
    window at column x of the mirror image is the window at Wr - crop - x of the image, mirrored"""
    cl, ct = pp.crop_offset(Wr, crop), pp.crop_offset(Hr, crop)
    wins = [(0, 0), (Wr - crop, 0), (0, Hr - crop), (Wr - crop, Hr - crop), (cl, ct)]
    return [(i, 0, 0, w, h, Wr, Hr, Wr - crop - x if mirrored else x, y, int(mirrored)) for x, y in wins]


def five_crop_views(batch, size, crop):
    """five views per image, image-major: the corners of the resized image (at 0 and dim - crop) in the order top-left, top-right,
    bottom-left, bottom-right, then the centre crop (`preprocess.crop_offset`)"""
    rows = []
    for i, (h, w) in enumerate(_sides(batch)):
        Hr, Wr = _resized(i, h, w, size, crop)
        rows += _five(i, h, w, Hr, Wr, crop, False)
    return make_views(rows)


def ten_crop_views(batch, size, crop):
    """ten views per image, image-major: the five of `five_crop_views`, then the five crops of the MIRRORED resized image in the
    same order — the mirrored views of top-right, top-left, bottom-right, bottom-left and of the window at Wr - crop - centre
    (the centre itself where Wr - crop is even)"""
    rows = []
    for i, (h, w) in enumerate(_sides(batch)):
        Hr, Wr = _resized(i, h, w, size, crop)
        rows += _five(i, h, w, Hr, Wr, crop, False) + _five(i, h, w, Hr, Wr, crop, True)
    return make_views(rows)


def box_views(image, boxes, crop, mode="stretch", size=None, flip=False):
    """one view per box of image number `image`; boxes: rows of (x0, y0, bw, bh).  mode "stretch": the box resized to crop x crop
    whatever its shape (rw = rh = crop, the window at 0: resized_crop's geometry).  mode "short": the eval rule applied to the box
    as if it were an image — its shorter side becomes `size` (default: crop), then the centre crop."""
    if mode not in ("stretch", "short"):
        raise ValueError(f"mode = {mode!r}: 'stretch' or 'short'")
    rows = []
    for j, (x0, y0, bw, bh) in enumerate(np.asarray(boxes, dtype=np.int64).reshape(-1, 4).tolist()):
        if bw < 1 or bh < 1:
            raise ValueError(f"box {j}: empty")
        if mode == "stretch":
            rows.append((image, x0, y0, bw, bh, crop, crop, 0, 0, int(flip)))
        else:
            Hr, Wr = pp.resized_size(bh, bw, crop if size is None else size)
            if crop > Hr or crop > Wr:
                raise ValueError(f"box {j}: crop {crop} larger than the resized box {Hr} x {Wr}")
            rows.append((image, x0, y0, bw, bh, Wr, Hr, pp.crop_offset(Wr, crop), pp.crop_offset(Hr, crop), int(flip)))
    return make_views(rows)


def random_resized_crop_views(batch, crop, rng, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), flip_p=0.5, per_image=1):
    """`per_image` random views of every image, image-major, drawn from the numpy Generator `rng`: a box of `scale` of the image's
    area (uniform) and of an aspect ratio w / h in `ratio` (log-uniform), placed uniformly; ten tries per view, then the central
    fallback (the whole image, or the largest centred box of the nearest allowed ratio); the box stretched to crop x crop; mirrored
    with probability flip_p.  The same generator state gives the same table."""
    rows = []
    lo, hi = np.log(ratio[0]), np.log(ratio[1])
    for i, (h, w) in enumerate(_sides(batch)):
        for _ in range(per_image):
            box = None
            for _try in range(10):
                target = h * w * rng.uniform(scale[0], scale[1])
                aspect = np.exp(rng.uniform(lo, hi))
                bw, bh = int(round(np.sqrt(target * aspect))), int(round(np.sqrt(target / aspect)))
                if 0 < bw <= w and 0 < bh <= h:
                    box = (int(rng.integers(0, w - bw + 1)), int(rng.integers(0, h - bh + 1)), bw, bh)
                    break
            if box is None:
                if w / h < ratio[0]:
                    bw, bh = w, min(h, max(1, int(round(w / ratio[0]))))
                elif w / h > ratio[1]:
                    bw, bh = min(w, max(1, int(round(h * ratio[1])))), h
                else:
                    bw, bh = w, h
                box = ((w - bw) // 2, (h - bh) // 2, bw, bh)
            rows.append((i,) + box + (crop, crop, 0, 0, int(rng.random() < flip_p)))
    return make_views(rows)


def check_views(sides, views, crop):
    """the per-view checks of the C entries on the host (include/ivit_views.h); ValueError names the view"""
    for j, v in enumerate(views):
        if not 0 <= v["image"] < len(sides):
            raise ValueError(f"view {j}: image outside the image table")
        h, w = sides[int(v["image"])]
        if v["bw"] < 1 or v["bh"] < 1 or v["x0"] < 0 or v["y0"] < 0 or int(v["x0"]) + int(v["bw"]) > w or int(v["y0"]) + int(v["bh"]) > h:
            raise ValueError(f"view {j}: box outside the image")
        if not (1 <= v["rw"] <= 65536 and 1 <= v["rh"] <= 65536):
            raise ValueError(f"view {j}: resized size outside 1 .. 65536")
        if v["left"] < 0 or v["top"] < 0 or int(v["left"]) + crop > v["rw"] or int(v["top"]) + crop > v["rh"]:
            raise ValueError(f"view {j}: window outside the resized box")
        if v["flip"] not in (0, 1):
            raise ValueError(f"view {j}: flip must be 0 or 1")


def views_reference(images, views, crop):
    """The contract of ivit_view_resize_u8_pil in numpy: a list of uint8 [h, w, 3] arrays and a view table -> uint8 [V, crop, crop,
    3], the bytes of PIL's crop(box).resize((rw, rh), BICUBIC).crop(window), mirrored where flip is set.  The box is resampled as an
    image of its own (`preprocess.pil_resize_center_crop_reference`'s passes on the sub-array, with (rw, rh) and the window given):
    horizontal pass first, into uint8, for the window's columns and the box's rows the window's vertical taps reach; then the
    vertical pass; an axis whose length does not change is copied."""
    views = np.ascontiguousarray(views, dtype=VIEW_DTYPE)
    crop = int(crop)
    if crop < 1:
        raise ValueError("crop must be positive")
    images = [np.asarray(im) for im in images]
    check_views([im.shape[:2] for im in images], views, crop)
    out = np.empty((len(views), crop, crop, 3), np.uint8)
    for j, v in enumerate(views):
        im = images[int(v["image"])]
        assert im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3
        x0, y0, bw, bh, rw, rh, left, top = (int(v[n]) for n in VIEW_FIELDS[1:9])
        box = im[y0:y0 + bh, x0:x0 + bw]
        if rh == bh:
            r0, r1 = top, top + crop
        else:
            lo, hi = pp.pil_coefficients(bh, rh, top), pp.pil_coefficients(bh, rh, top + crop - 1)
            r0, r1 = lo[0], hi[0] + len(hi[1])
        rows = np.ascontiguousarray(box[r0:r1].transpose(1, 0, 2))                     # [bw, rows, 3]
        hor = pp._pil_pass(rows, bw, rw, left, crop).transpose(1, 0, 2)                 # [rows, crop, 3]
        if rh == bh:
            res = hor
        else:
            full = np.zeros((bh, crop, 3), np.uint8)
            full[r0:r1] = hor
            res = pp._pil_pass(full, bh, rh, top, crop)
        out[j] = res[:, ::-1] if v["flip"] else res
    return out


def _view_args(batch, views):
    """(arguments of the view entries up to V, keep-alive): the view table is uploaded once per call"""
    if not isinstance(batch, pp.RaggedImages) or len(batch) == 0:
        raise TypeError("expected a non-empty RaggedImages (pack_images)")
    views = np.ascontiguousarray(views, dtype=VIEW_DTYPE)
    dev = torch.from_numpy(views.view(np.uint8).copy()).to(batch.pixels.device) if len(views) else None
    args = (ctypes.c_void_p(batch.pixels.data_ptr()), ctypes.c_size_t(batch.pixels.numel()),
            batch.desc.ctypes.data_as(ctypes.POINTER(_lib.ImageDesc)), ctypes.c_void_p(batch.desc_dev.data_ptr()), len(batch),
            views.ctypes.data_as(ctypes.POINTER(_lib.ViewDesc)) if len(views) else None,
            ctypes.c_void_p(dev.data_ptr()) if len(views) else None, len(views))
    return args, (views, dev)


def view_resize(batch, views, crop):
    """RaggedImages and a view table -> uint8 [V, crop, crop, 3] on the batch's device: PIL's bytes of every view, one launch
    (ivit_view_resize_u8_pil)"""
    args, keep = _view_args(batch, views)
    out = torch.empty(len(keep[0]), crop, crop, 3, dtype=torch.uint8, device=batch.pixels.device)
    if len(keep[0]):                                    # no views: nothing to launch
        handle(out.device).call("ivit_view_resize_u8_pil", *args, int(crop), ctypes.c_void_p(out.data_ptr()))
    return out


def view_transform(batch, views, scale, crop, mean=pp.IMAGENET_DEFAULT_MEAN, std=pp.IMAGENET_DEFAULT_STD):
    """RaggedImages and a view table -> int8 [V, 3, crop, crop]: every view through ToTensor, Normalize and the input QuantAct of
    scale `scale`, one launch (ivit_view_transform_u8) — what `engine.forward` takes; the uint8 crops are never written"""
    args, keep = _view_args(batch, views)
    out = torch.empty(len(keep[0]), 3, crop, crop, dtype=torch.int8, device=batch.pixels.device)
    m = (ctypes.c_float * 3)(*[float(np.float32(v)) for v in mean])
    s = (ctypes.c_float * 3)(*[float(np.float32(v)) for v in std])
    if len(keep[0]):
        handle(out.device).call("ivit_view_transform_u8", *args, int(crop), m, s, float(np.float32(scale)), ctypes.c_void_p(out.data_ptr()))
    return out
