"""Timing of the uint8 front end on the device (profiles/README.md, "The PIL-exact ragged front end"):
  * 256 images of 500 x 375, size 256, crop 224: ONE launch of ivit_eval_transform_u8 beside the parent chain on the same pixels,
    ivit_resize_center_crop_u8 (two launches, an fp32 workspace) + ivit_normalize_quantize_u8;
  * 256 images with both sides drawn from 200 .. 800: one launch of ivit_eval_transform_u8 beside the only form the torch-pinned
    entries have for images of different sizes, 256 B = 1 chains.
Medians of HIP-event times with quartiles and extremes; the variants of one comparison alternate inside one loop.  All buffers are
allocated before the timed loops.  Prints a box probe line, then one JSON line per comparison.
    python tools/front_end_bench.py [--reps 30]"""
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
from topk_bench import interleaved  # noqa: E402

_P = ctypes.c_void_p
SIZE, CROP, SCALE = 256, 224, 0.0207


def f3(v):
    return (ctypes.c_float * 3)(*[float(np.float32(x)) for x in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    B = args.batch
    prop = torch.cuda.get_device_properties(0)
    print(json.dumps({"what": "box", "device": prop.name, "cus": prop.multi_processor_count, "torch": torch.__version__,
                      "hip": torch.version.hip}), flush=True)
    H = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    mean, std = f3(pp.IMAGENET_DEFAULT_MEAN), f3(pp.IMAGENET_DEFAULT_STD)
    gen = torch.Generator(device="cuda").manual_seed(5)
    rng = np.random.Generator(np.random.PCG64(5))
    out_new = torch.empty(B, 3, CROP, CROP, dtype=torch.int8, device="cuda")
    out_old = torch.empty(B, 3, CROP, CROP, dtype=torch.int8, device="cuda")
    crop_u8 = torch.empty(B, CROP, CROP, 3, dtype=torch.uint8, device="cuda")

    def new_launch(rag):
        a = (_P(rag.pixels.data_ptr()), rag.pixels.numel(), rag.desc.ctypes.data_as(ctypes.POINTER(_lib.ImageDesc)),
             _P(rag.desc_dev.data_ptr()), len(rag), SIZE, CROP, mean, std, SCALE, _P(out_new.data_ptr()))
        return lambda: H.call("ivit_eval_transform_u8", *a)

    def chain(ptr, n, h, w, ws, u8, out):
        a = (_P(ptr), n, h, w, SIZE, CROP, _P(ws.data_ptr()), _P(u8))
        b = (_P(u8), n, CROP, CROP, mean, std, SCALE, _P(out))
        def run():
            H.call("ivit_resize_center_crop_u8", *a)
            H.call("ivit_normalize_quantize_u8", *b)
        return run

    for what, shapes in (("equal sizes 375 x 500", [(375, 500)] * B),
                         ("ragged, sides 200 .. 800", [tuple(int(v) for v in rng.integers(200, 801, 2)) for _ in range(B)])):
        sizes = np.array([h * w * 3 for h, w in shapes], np.int64)
        desc = np.zeros(B, pp.DESC_DTYPE)
        desc["offset"], desc["h"], desc["w"] = np.cumsum(sizes) - sizes, [s[0] for s in shapes], [s[1] for s in shapes]
        pixels = torch.randint(0, 256, (int(sizes.sum()),), dtype=torch.uint8, device="cuda", generator=gen)
        rag = pp.RaggedImages(pixels, desc)
        variants = {"ivit_eval_transform_u8, one launch": new_launch(rag)}
        if len(set(shapes)) == 1:
            h, w = shapes[0]
            ws = torch.empty(B * h * CROP * 3, dtype=torch.float32, device="cuda")
            variants["parent chain, one batch"] = chain(pixels.data_ptr(), B, h, w, ws, crop_u8.data_ptr(), out_old.data_ptr())
        else:
            ws = torch.empty(max(s[0] for s in shapes) * CROP * 3, dtype=torch.float32, device="cuda")
            calls = [chain(pixels.data_ptr() + int(d["offset"]), 1, int(d["h"]), int(d["w"]), ws, crop_u8.data_ptr() + i * CROP * CROP * 3,
                           out_old.data_ptr() + i * 3 * CROP * CROP) for i, d in enumerate(desc)]
            variants["parent chain, B = 1 per image"] = lambda: [c() for c in calls]
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        # the two front ends differ where PIL's filter differs from torch's: reported, not asserted; the new launch against the numpy
        # statement of PIL on the first two images
        want = pp.pil_resize_center_crop_reference([pixels[int(d["offset"]):int(d["offset"]) + int(d["h"]) * int(d["w"]) * 3]
                                                    .reshape(int(d["h"]), int(d["w"]), 3).cpu().numpy() for d in desc[:2]], SIZE, CROP)
        ref = pp.normalize_quantize(torch.from_numpy(want).cuda(), SCALE)
        t, _ = interleaved(variants, args.reps, warmup=3)
        print(json.dumps({"what": what, "batch": B, "size": SIZE, "crop": CROP, "input_MB": round(float(sizes.sum()) / 1e6, 1), "us": t,
                          "new_equals_pil_reference_on_2_images": bool(torch.equal(out_new[:2], ref)),
                          "bytes_differing_from_torch_pinned_chain": int((out_new != out_old).sum()), "of": out_new.numel()}), flush=True)


if __name__ == "__main__":
    main()
