"""Timing of the image views (profiles/README.md, "Image views"):
  * the A/B of the shared kernel body: ivit_eval_transform_u8 of THIS library beside the same entry of another build of the library
    (--base PATH: the parent commit's libivit_hip.so), 256 images of 500 x 375 and 256 ragged ones, size 256, crop 224.  The base runs
    TWICE in every round (first and last), so the difference of its two medians is the spread the base shows against itself in the
    same session: the margin the comparison has;
  * a ten-crop of 256 images (2560 views, size 256, crop 224): ONE launch of ivit_view_transform_u8 beside ten launches of
    ivit_eval_transform_u8 on the same images (ten times centre-sized work, the only form there was), and the centre views alone
    through both entries.
Medians of HIP-event times with quartiles and extremes; the variants of one comparison alternate inside one loop.  All buffers are
allocated before the timed loops.  Prints a box line, then one JSON line per comparison.
    python tools/views_bench.py [--base /path/to/parent/libivit_hip.so] [--reps 30]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ivit_amd import _lib  # noqa: E402
from ivit_amd import preprocess as pp  # noqa: E402
from ivit_amd import views as vw  # noqa: E402
from topk_bench import interleaved  # noqa: E402

_P = ctypes.c_void_p
SIZE, CROP, SCALE = 256, 224, 0.0207


def f3(v):
    return (ctypes.c_float * 3)(*[float(np.float32(x)) for x in v])


class BaseHandle:
    """ivit_create / ivit_eval_transform_u8 of another build of the library, bound by the same header"""
    def __init__(self, path, stream):
        self.lib = _lib.bind(ctypes.CDLL(path), names=["create", "destroy", "eval_transform_u8", "last_error"])
        self.h = _P()
        assert self.lib.ivit_create(ctypes.byref(self.h), 0, _P(stream)) == 0

    def call(self, name, *args):
        st = getattr(self.lib, name)(self.h, *args)
        assert st == 0, (name, st, self.lib.ivit_last_error(self.h).decode())


def ragged(shapes, gen):
    sizes = np.array([h * w * 3 for h, w in shapes], np.int64)
    desc = np.zeros(len(shapes), pp.DESC_DTYPE)
    desc["offset"], desc["h"], desc["w"] = np.cumsum(sizes) - sizes, [s[0] for s in shapes], [s[1] for s in shapes]
    pixels = torch.randint(0, 256, (int(sizes.sum()),), dtype=torch.uint8, device="cuda", generator=gen)
    return pp.RaggedImages(pixels, desc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--base", default=None, help="another build of libivit_hip.so (the parent commit's) for the A/B of ivit_eval_transform_u8")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    B = args.batch
    prop = torch.cuda.get_device_properties(0)
    print(json.dumps({"what": "box", "device": prop.name, "cus": prop.multi_processor_count, "torch": torch.__version__,
                      "hip": torch.version.hip}), flush=True)
    stream = torch.cuda.current_stream().cuda_stream
    H = _lib.Handle(0, stream)
    base = BaseHandle(args.base, stream) if args.base else None
    mean, std = f3(pp.IMAGENET_DEFAULT_MEAN), f3(pp.IMAGENET_DEFAULT_STD)
    gen = torch.Generator(device="cuda").manual_seed(5)
    rng = np.random.Generator(np.random.PCG64(5))
    out = torch.empty(B, 3, CROP, CROP, dtype=torch.int8, device="cuda")
    out_base = torch.empty(B, 3, CROP, CROP, dtype=torch.int8, device="cuda")
    out_views = torch.empty(10 * B, 3, CROP, CROP, dtype=torch.int8, device="cuda")

    def eval_args(rag, dst):
        return (_P(rag.pixels.data_ptr()), rag.pixels.numel(), rag.desc.ctypes.data_as(ctypes.POINTER(_lib.ImageDesc)),
                _P(rag.desc_dev.data_ptr()), len(rag), SIZE, CROP, mean, std, SCALE, _P(dst))

    def view_args(rag, table, table_dev, dst):
        return (_P(rag.pixels.data_ptr()), rag.pixels.numel(), rag.desc.ctypes.data_as(ctypes.POINTER(_lib.ImageDesc)),
                _P(rag.desc_dev.data_ptr()), len(rag), table.ctypes.data_as(ctypes.POINTER(_lib.ViewDesc)), _P(table_dev.data_ptr()),
                len(table), CROP, mean, std, SCALE, _P(dst))

    sets = (("equal sizes 375 x 500", [(375, 500)] * B),
            ("ragged, sides 200 .. 800", [tuple(int(v) for v in rng.integers(200, 801, 2)) for _ in range(B)]))
    for what, shapes in sets:
        rag = ragged(shapes, gen)
        a = eval_args(rag, out.data_ptr())
        # ---- the A/B of ivit_eval_transform_u8
        if base is not None:
            ab = eval_args(rag, out_base.data_ptr())
            variants = {"base, first": lambda: base.call("ivit_eval_transform_u8", *ab),
                        "this library": lambda: H.call("ivit_eval_transform_u8", *a),
                        "base, last": lambda: base.call("ivit_eval_transform_u8", *ab)}
            t, _ = interleaved(variants, args.reps, warmup=3)
            print(json.dumps({"what": "A/B ivit_eval_transform_u8, " + what, "batch": B, "us": t,
                              "this_minus_base_us": round(t["this library"]["median"] - min(t["base, first"]["median"], t["base, last"]["median"]), 2),
                              "base_against_itself_us": round(abs(t["base, first"]["median"] - t["base, last"]["median"]), 2),
                              "same_bytes": bool(torch.equal(out, out_base))}), flush=True)
        # ---- the centre views through both entries, and the ten-crop
        center, ten = vw.center_views(rag, SIZE, CROP), vw.ten_crop_views(rag, SIZE, CROP)
        center_dev, ten_dev = (torch.from_numpy(t.view(np.uint8).copy()).cuda() for t in (center, ten))
        ac = view_args(rag, center, center_dev, out_views.data_ptr())
        at = view_args(rag, ten, ten_dev, out_views.data_ptr())
        tens = [eval_args(rag, out_views.data_ptr() + j * B * 3 * CROP * CROP) for j in range(10)]
        H.call("ivit_view_transform_u8", *ac)
        H.call("ivit_eval_transform_u8", *a)
        torch.cuda.synchronize()
        same = bool(torch.equal(out_views[:B], out))
        variants = {"ivit_eval_transform_u8, centre": lambda: H.call("ivit_eval_transform_u8", *a),
                    "ivit_view_transform_u8, centre views": lambda: H.call("ivit_view_transform_u8", *ac),
                    "ivit_view_transform_u8, ten-crop in one launch": lambda: H.call("ivit_view_transform_u8", *at),
                    "ivit_eval_transform_u8, ten launches": lambda: [H.call("ivit_eval_transform_u8", *x) for x in tens]}
        t, _ = interleaved(variants, args.reps, warmup=3)
        print(json.dumps({"what": "views, " + what, "batch": B, "views": len(ten), "size": SIZE, "crop": CROP, "us": t,
                          "centre_views_equal_eval_transform": same}), flush=True)


if __name__ == "__main__":
    main()
