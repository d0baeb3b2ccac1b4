"""Files -> int8 [B, 3, 224, 224] in images/s, three paths on one box, interleaved (include/ivit_jpeg.h, include/ivit_jpeg_entropy.h,
ivit_amd/jpeg.py):

  pil      Pillow decodes every file on a pool of T threads, pack_images uploads the pixels, ivit_eval_transform_u8
  native   jpeg.decode (entropy decode on T threads, one pinned copy, the device reconstruction), ivit_eval_transform_u8
  device   jpeg.decode(entropy="device") (the pre-pass on T threads, the Huffman decode and the reconstruction on the device), the same

the device entropy decode's one launch alone at every subsequence size of --bits (HIP events, medians, interleaved), and, separately, the reconstruction's two launches alone against the bytes they move (coefficients in, planes out and in, pixels
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
    ap.add_argument("--bits", type=int, nargs="+", default=[128, 256, 512, 1024, 2048, 4096], help="subsequence sizes of the sweep")
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

    def path_device(t):
        batch, fb = J.decode(files, "cuda", threads=t, entropy="device")
        assert not fb
        out = pp.eval_transform_pil(batch, scale, size, crop)
        torch.cuda.synchronize()
        return out

    want = path_pil(8)
    assert torch.equal(want, path_native(8)) and torch.equal(want, path_device(8))     # the same bytes, and all paths warm
    for t in args.threads:
        times = {"pil": [], "native": [], "device": []}
        for _ in range(args.rounds):                                  # interleaved: drift of the box hits all alike
            for name, fn in (("pil", path_pil), ("native", path_native), ("device", path_device)):
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

    # the device entropy decode alone: one launch per batch, every subsequence size in turn round by round
    scans = [J.scan(f) for f in files]
    dtab, nc_e, _, _ = J.layout([x[0] for x in scans], [x[4] for x in scans], [x[5] for x in scans])
    stab, segs, nstream, wsb = J.entropy_layout([x[1] for x in scans], [x[3] for x in scans])
    streams = np.zeros(nstream, np.uint8)
    for k, x in enumerate(scans):
        streams[stab[k].stream_offset:][:len(x[2])] = x[2]
    n = len(files)
    dev = [torch.from_numpy(a.copy()).cuda() for a in (streams, np.frombuffer(dtab, np.uint8, n * 264), np.frombuffer(stab, np.uint8, n * 6008),
                                                       segs.view(np.uint8))]
    e_coefs, e_work = torch.empty(nc_e, dtype=torch.int16, device="cuda"), torch.empty(wsb, dtype=torch.uint8, device="cuda")
    e_status = torch.empty(n, dtype=torch.int32, device="cuda")

    def entropy(bits):
        J.entropy_decode_device(dev[0], dtab, dev[1], stab, dev[2], segs, dev[3], n, e_work, e_coefs, e_status, bits)

    sweep = {b: [] for b in [0] + args.bits}
    for b in sweep:                                                   # warm, and the host decoder's coefficients at every size
        entropy(b)
        torch.cuda.synchronize()
        assert not e_status.any().item()
        got = e_coefs.cpu().numpy()
        for k in range(0, n, max(1, n // 8)):
            assert np.array_equal(got[dtab[k].coef_offset:][:scans[k][4]], J.entropy_decode(files[k])[1])
    for _ in range(max(args.rounds, 5)):
        for b in sweep:
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            entropy(b)
            z.record()
            torch.cuda.synchronize()
            sweep[b].append(a.elapsed_time(z) * 1e3)
    for b, us in sweep.items():
        res["entropy_device_bits%d_us" % b] = round(statistics.median(us), 1)
        res["entropy_device_bits%d_spread" % b] = round((max(us) - min(us)) / statistics.median(us), 3)
    res["entropy_device_images_per_s"] = round(n / statistics.median(sweep[0]) * 1e6)
    res["stream_bytes_mean"] = int(np.mean([len(x[2]) for x in scans]))
    t0 = time.perf_counter()
    for f in files:
        J.scan(f)
    res["one_core_scan_images_per_s"] = round(n / (time.perf_counter() - t0), 1)

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
