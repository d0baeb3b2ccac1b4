"""Writes tests/golden/pil_resize.npz: the pin of the PIL-exact ragged front end (ivit_resize_center_crop_u8_pil,
ivit_eval_transform_u8, ivit_amd.preprocess.pil_resize_center_crop_reference).  Needs Pillow; deterministic (seeded PCG64, like
ivit_amd.synth); the Pillow version is recorded in the file.

    python tools/make_pil_resize_fixture.py

The file holds the packed uint8 HWC images (`pixels`, `offsets` int64 [N], `shapes` int32 [N, 2] = (h, w)), `cases` int32 [C, 2] =
(size, crop), and per case c the indices of its images (`case{c}_images`) and PIL's own output for them (`case{c}_out` uint8
[n, crop, crop, 3]): Image.resize((Wr, Hr), Image.BICUBIC).crop(...), with torchvision's sizes and offsets.
Contents (tests/test_pil_resize_cpu.py asserts each class from the descriptors): portrait and landscape down-scales, an up-scale,
short side == size in either orientation (both passes skipped: the bytes are copied), a square with size == crop, odd (Hr - crop) and (Wr - crop) whose half lands
on an even and on an odd integer, 1-pixel strips, images on both sides of the tiled / streaming switch (vertical tap count 96),
crops of two full 32-row bands plus a partial one and of a single partial band, random and saturated 0 / 255 pixels."""
import os
import sys

import numpy as np
from PIL import Image
import PIL

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ivit_amd.preprocess import crop_offset, resized_size  # noqa: E402

SEED = 20240611
# (size, crop) -> [(h, w, kind)]; kind "r" random pixels, "s" saturated 0 / 255
CASES = [
    ((80, 72), [(96, 120, "r"), (118, 90, "s"), (40, 52, "r"), (80, 111, "r"), (100, 80, "s"), (80, 80, "r"),
                (80, 85, "r"), (80, 87, "s"), (85, 80, "r"), (87, 80, "r")]),
    ((24, 20), [(100, 120, "r"), (30, 1, "s"), (1, 25, "r"), (61, 37, "s")]),
    ((32, 32), [(57, 57, "r"), (32, 32, "s")]),
    ((4, 3), [(94, 110, "r"), (95, 110, "s"), (120, 100, "r"), (92, 100, "s")]),
    # a micro model's input (32 px) from five sizes: the end-to-end test cuts ragged batches from these
    ((36, 32), [(40, 44, "r"), (50, 38, "r"), (36, 60, "s"), (45, 45, "r"), (70, 41, "r")]),
]


def main():
    rng = np.random.Generator(np.random.PCG64(SEED))
    images, out = [], {}
    cases = []
    for c, ((size, crop), specs) in enumerate(CASES):
        idx, res = [], []
        for h, w, kind in specs:
            if kind == "r":
                im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            else:
                im = (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
            Hr, Wr = resized_size(h, w, size)
            top, left = crop_offset(Hr, crop), crop_offset(Wr, crop)
            pil = Image.fromarray(im, "RGB").resize((Wr, Hr), Image.BICUBIC).crop((left, top, left + crop, top + crop))
            res.append(np.asarray(pil))
            idx.append(len(images))
            images.append(im)
        cases.append((size, crop))
        out[f"case{c}_images"] = np.array(idx, np.int32)
        out[f"case{c}_out"] = np.stack(res)
    sizes = np.array([im.size for im in images], np.int64)
    out.update(pixels=np.concatenate([im.reshape(-1) for im in images]), offsets=np.cumsum(sizes) - sizes,
               shapes=np.array([im.shape[:2] for im in images], np.int32), cases=np.array(cases, np.int32),
               pillow_version=np.array(PIL.__version__), seed=np.int64(SEED))
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "pil_resize.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(images), "images, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
