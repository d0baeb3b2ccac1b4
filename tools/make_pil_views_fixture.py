"""Writes tests/golden/pil_views.npz: the pin of the image views (ivit_view_resize_u8_pil, ivit_view_transform_u8,
ivit_amd.views.views_reference).  Needs Pillow; the Pillow version is recorded in the file.

    python tools/make_pil_views_fixture.py

The file holds NO pixels of its own: its views are over the images of tests/golden/pil_resize.npz (tools/make_pil_resize_fixture.py),
named by their index there.  `views` int32 [N, 10] in the order of ivit_amd.views.VIEW_FIELDS, `crops` int32 [N] the crop of every
view, `bytes` uint8: Pillow's output of every view, [crop, crop, 3] each, back to back —
    Image.crop((x0, y0, x0 + bw, y0 + bh)).resize((rw, rh), Image.BICUBIC).crop((left, top, left + crop, top + crop))
and .transpose(Image.FLIP_LEFT_RIGHT) where flip is set.  `tencrop` int32 [4] = (image, size, crop, first view): ten of the views are
the ten-crop of one image, and THEIR bytes are Pillow's crops of the resized image and of its mirror image taken by hand, not
through the view descriptors.
Contents (tests/test_views_cpu.py asserts each class from the descriptors): an up-scale and a down-scale on each axis, axes that are
copied, a 1-pixel-wide and a 1-pixel-high box, boxes touching each edge of their image, the whole image, windows at all four corners
of the resized box, mirrored views with an odd and an even crop, crop 1, saturated 0 / 255 images, the ten-crop."""
import os
import sys

import numpy as np
from PIL import Image
import PIL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ivit_amd.preprocess import resized_size  # noqa: E402
from ivit_amd.views import ten_crop_views  # noqa: E402

# crop -> [(image, x0, y0, bw, bh, rw, rh, left, top, flip)]; the images (h x w): 0 96x120, 1 118x90 saturated, 2 40x52, 3 80x111,
# 4 100x80 saturated, 5 80x80, 7 80x87 saturated, 10 100x120, 11 30x1 saturated, 13 61x37 saturated, 16 94x110, 18 120x100, 19 92x100 saturated
VIEWS = {
    16: [(0, 10, 7, 90, 80, 40, 30, 3, 2, 0),          # down-scale on both axes, a box inside the image
         (2, 5, 6, 12, 10, 30, 25, 14, 9, 0),          # up-scale on both axes; the window at the bottom-right corner
         (3, 0, 0, 10, 70, 20, 18, 4, 0, 0),           # up on x, down on y; touches the left and the top edge; top-right corner
         (16, 10, 84, 100, 10, 25, 20, 0, 4, 1),       # down on x, up on y; touches the right and the bottom edge; bottom-left; mirrored
         (4, 3, 3, 50, 60, 24, 28, 0, 0, 0),           # the window at the top-left corner, a saturated image
         (5, 8, 8, 40, 33, 40, 20, 5, 2, 0),           # the horizontal axis copied
         (5, 1, 2, 33, 40, 18, 40, 1, 20, 1),          # the vertical axis copied, mirrored
         (7, 4, 4, 20, 22, 20, 22, 2, 3, 0),           # both axes copied: the bytes of a saturated image
         (11, 0, 0, 1, 30, 16, 16, 0, 0, 0),           # a 1-pixel-wide image, whole
         (0, 50, 10, 1, 40, 17, 20, 1, 3, 0),          # a 1-pixel-wide box inside an image
         (0, 20, 30, 60, 1, 20, 16, 2, 0, 1),          # a 1-pixel-high box
         (13, 0, 0, 37, 61, 20, 33, 2, 8, 1)],         # the whole image, mirrored with an even crop
    7: [(18, 7, 9, 80, 100, 9, 11, 1, 2, 0),           # a down-scale of 9
        (18, 7, 9, 80, 100, 9, 11, 1, 2, 1),           # the same, mirrored with an odd crop
        (1, 0, 0, 90, 118, 12, 7, 5, 0, 1)],           # the whole of a saturated image
    1: [(10, 0, 0, 120, 100, 1, 1, 0, 0, 0),           # crop 1: a whole image into one pixel
        (19, 30, 40, 5, 3, 4, 2, 3, 1, 1)],
}
TENCROP = (20, 21, 16)                                 # image 20 (40 x 44) at size 21 -> 21 x 23: both (dim - crop) odd


def pil_view(im, v, crop):
    image, x0, y0, bw, bh, rw, rh, left, top, flip = v
    out = Image.fromarray(im, "RGB").crop((x0, y0, x0 + bw, y0 + bh)).resize((rw, rh), Image.BICUBIC).crop((left, top, left + crop, top + crop))
    return np.asarray(out.transpose(Image.FLIP_LEFT_RIGHT) if flip else out)


def main():
    g = np.load(os.path.join(ROOT, "tests", "golden", "pil_resize.npz"))
    images = [g["pixels"][o:o + int(h) * int(w) * 3].reshape(int(h), int(w), 3) for o, (h, w) in zip(g["offsets"], g["shapes"])]
    views, crops, res = [], [], []
    for crop, rows in VIEWS.items():
        for v in rows:
            views.append(v)
            crops.append(crop)
            res.append(pil_view(images[v[0]], v, crop))
    # the ten-crop by hand: five crops of the resized image, five of its mirror image
    image, size, crop = TENCROP
    im = images[image]
    Hr, Wr = resized_size(im.shape[0], im.shape[1], size)
    resized = Image.fromarray(im, "RGB").resize((Wr, Hr), Image.BICUBIC)
    cl, ct = int(np.rint((Wr - crop) / 2.0)), int(np.rint((Hr - crop) / 2.0))
    first = len(views)
    table = ten_crop_views([im.shape[:2]], size, crop)
    table["image"] = image
    for j, pic in enumerate((resized, resized.transpose(Image.FLIP_LEFT_RIGHT))):
        for k, (x, y) in enumerate(((0, 0), (Wr - crop, 0), (0, Hr - crop), (Wr - crop, Hr - crop), (cl, ct))):
            views.append(tuple(int(t) for t in table[5 * j + k]))
            crops.append(crop)
            res.append(np.asarray(pic.crop((x, y, x + crop, y + crop))))
    path = os.path.join(ROOT, "tests", "golden", "pil_views.npz")
    np.savez_compressed(path, views=np.array(views, np.int32), crops=np.array(crops, np.int32),
                        bytes=np.concatenate([r.reshape(-1) for r in res]), tencrop=np.array(TENCROP + (first,), np.int32),
                        pillow_version=np.array(PIL.__version__))
    print("wrote", path, os.path.getsize(path), "bytes,", len(views), "views, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
