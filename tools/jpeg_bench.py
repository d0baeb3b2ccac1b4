"""Files -> int8 [B, 3, 224, 224] in images/s, two paths on one box, interleaved (include/ivit_jpeg.h, ivit_amd/jpeg.py):

  pil      Pillow decodes every file on a pool of T threads, pack_images uploads the pixels, ivit_eval_transform_u8
  native   jpeg.decode (entropy decode on T threads, one pinned copy, the device reconstruction), ivit_eval_transform_u8

and, separately, the reconstruction's two launches alone against the bytes they move (coefficients in, planes out and in, pixels
out), with the fraction of the HBM rate (--hbm-gbs, default 8000) that implies, and the host entropy decode alone per core against
Pillow's whole decode per core.

    python tools/jpeg_bench.py --images 256 --threads 8 16 --rounds 7

The files are synthetic, written by Pillow: --width x --height (500 x 375), 4:2:0, quality 90, a smooth random field with fine noise on
it so that the entropy-coded size is that of a photograph.  Prints one JSON line."""
import argparse
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ivit_amd import jpeg as J  # noqa: E402
from ivit_amd import preprocess as pp  # noqa: E402


def synth(n, w, h, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        low = rng.integers(0, 256, size=(h // 25 + 2, w // 25 + 2, 3), dtype=np.uint8)
        im = np.asarray(Image.fromarray(low).resize((w, h), Image.BICUBIC)).astype(np.int16)
        im = np.clip(im + rng.normal(0, 6, size=im.shape), 0, 255).astype(np.uint8)
        f = io.BytesIO()
        Image.fromarray(im).save(f, "JPEG", quality=90, subsampling=2)
        out.append(f.getvalue())
    return out


def pil_decode(d):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--width", type=int, default=500)
    ap.add_argument("--height", type=int, default=375)
    ap.add_argument("--threads", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/jpeg_bench.py needs a HIP device")
    files = synth(args.images, args.width, args.height)
    scale, size, crop = 0.02, 256, 224
    res = {"images": args.images, "w": args.width, "h": args.height, "file_bytes_mean": int(np.mean([len(f) for f in files]))}

    def path_pil(t):
        with ThreadPoolExecutor(t) as pool:
            ims = list(pool.map(pil_decode, files))
        out = pp.eval_transform_pil(pp.pack_images(ims, "cuda"), scale, size, crop)
        torch.cuda.synchronize()
        return out

    def path_native(t):
        batch, fb = J.decode(files, "cuda", threads=t)
        assert not fb
        out = pp.eval_transform_pil(batch, scale, size, crop)
        torch.cuda.synchronize()
        return out

    assert torch.equal(path_pil(8), path_native(8))                   # the same bytes, and both paths warm
    for t in args.threads:
        times = {"pil": [], "native": []}
        for _ in range(args.rounds):                                  # interleaved: drift of the box hits both alike
            for name, fn in (("pil", path_pil), ("native", path_native)):
                t0 = time.perf_counter()
                fn(t)
                times[name].append(time.perf_counter() - t0)
        for name in times:
            res["%s_t%d_images_per_s" % (name, t)] = round(args.images / statistics.median(times[name]), 1)
            res["%s_t%d_spread" % (name, t)] = round((max(times[name]) - min(times[name])) / statistics.median(times[name]), 3)

    # one core: the host entropy decode alone against Pillow's whole decode
    infos = [J.query(f) for f in files]
    buf = np.empty(max(i[1] for i in infos), np.int16)
    one = {"entropy": [], "pil": []}
    for _ in range(3):
        t0 = time.perf_counter()
        for f in files:
            J.entropy_decode(f, buf)
        one["entropy"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        for f in files:
            pil_decode(f)
        one["pil"].append(time.perf_counter() - t0)
    res["one_core_entropy_decode_images_per_s"] = round(args.images / min(one["entropy"]), 1)
    res["one_core_pil_decode_images_per_s"] = round(args.images / min(one["pil"]), 1)

    # the reconstruction alone
    table, nc, npx, nws = J.layout([i[0] for i in infos], [i[1] for i in infos], [i[2] for i in infos])
    host = np.zeros(nc, np.int16)
    for j, f in enumerate(files):
        a = int(table[j].coef_offset)
        J.entropy_decode(f, host[a:a + infos[j][1]])
    coefs = torch.from_numpy(host).cuda()
    pixels = torch.empty(npx, dtype=torch.uint8, device="cuda")
    work = torch.empty(nws, dtype=torch.uint8, device="cuda")
    tdev = J.reconstruct(coefs, table, len(files), pixels, work)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
    for a, b in ev:
        a.record()
        J.reconstruct(coefs, table, len(files), pixels, work, table_dev=tdev)
        b.record()
    torch.cuda.synchronize()
    us = statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3
    moved = nc * 2 + 2 * nws + npx
    res.update(reconstruct_us=round(us, 1), reconstruct_bytes=moved, reconstruct_gbs=round(moved / us / 1e3, 1),
               hbm_fraction=round(moved / us / 1e3 / args.hbm_gbs, 3), reconstruct_images_per_s=round(args.images / us * 1e6))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
