"""Times the three launches of a k-means iteration SEPARATELY (include/ivit_cluster.h) and, beside them, the route a user has without
them on the same box: feat8.half() @ cent.half().T, the norm terms, argmax, index_add_.

    python tools/kmeans_bench.py [--rows 65536 1048576] [--dim 192 384 768] [--k 64 1024 16384] [--out kmeans_bench.json]

Per (rows, dim, K), on seeded blobs: device events around `reps` back-to-back calls of ONE entry after a warm-up of the same shape,
reps chosen so that a window lasts about --window seconds (at least 3 calls, no upper cap); the median of --repeat windows, and
beside every time its spread, [fastest window, slowest window], as `<name>_range`.  Reported:
  assign_ms, assign_tops, assign_frac   2 rows K dim integer operations over the time, and as a fraction of the int8 MFMA peak
                                        bench.py uses (INT8_PEAK_TOPS: 256 CU x 4 SIMD x 2048 OP/clk x 2.4 GHz)
  acc_ms, acc_gbs, acc_form             the accumulate, its added bytes per second (rows dim 8 bytes: one 64-bit add per feature)
                                        and which form ran (lds: the privatised copy; global: straight 64-bit atomics)
  update_ms                             the update
  torch_assign_ms, torch_acc_ms         the fp16 route, in row chunks that keep the [chunk, K] matrix below 2^28 elements (the
                                        whole matrix at 1 048 576 x 16 384 would be 32 GiB), and index_add_ + bincount into fp32 sums
The device results are compared with the numpy reference on the first 64 rows, and the totals with torch, before anything is timed.  Prints one JSON line
per shape and a markdown table at the end; needs a HIP device."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ivit_amd  # noqa: E402,F401
from ivit_amd import cluster as cl  # noqa: E402
from ivit_amd.predict import kmeans_assign_reference  # noqa: E402

INT8_PEAK_TOPS = 5033.0   # as bench.py: 256 CU x 4 SIMD x 2048 OP/clk x 2.4 GHz
_P = ctypes.c_void_p


def timed(fn, window, repeat):
    """(median, [min, max], reps): milliseconds per call of fn() over `repeat` windows of `reps` back-to-back calls between two device
    events, after a warm-up and one synchronised call that sizes the window (its host overhead counts, so a window of very short
    calls comes out somewhat shorter than `window`)"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    once = max(time.perf_counter() - t0, 1e-6)
    reps = int(max(3, window / once))
    out = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return statistics.median(out), [round(min(out), 4), round(max(out), 4)], reps


def blobs(rows, dim, K, seed):
    """seeded int8 blobs on the device: min(K, 4096) centres, sigma 12"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.randint(-90, 91, (min(K, 4096), dim), generator=g, device="cuda", dtype=torch.int32)
    which = torch.randint(0, centres.shape[0], (rows,), generator=g, device="cuda")
    x = centres[which] + (torch.randn(rows, dim, generator=g, device="cuda") * 12).round().to(torch.int32)
    x = x.clamp_(-128, 127).to(torch.int8)
    cent = x[torch.randperm(rows, generator=g, device="cuda")[:K]].contiguous() if K <= rows else None
    return x, cent


def torch_route(x, cent):
    """the route without the library: fp16 scores in row chunks, argmax, index_add_"""
    K = cent.shape[0]
    ch = cent.half()
    cn = (ch.float() ** 2).sum(1)
    step = max(1, (1 << 28) // K)
    parts = []
    for a in range(0, x.shape[0], step):
        s = 2.0 * (x[a:a + step].half() @ ch.T).float() - cn[None, :]
        parts.append(s.argmax(1))
    return torch.cat(parts)


def torch_accumulate(x, assign, sums, counts):
    sums.index_add_(0, assign, x.float())
    counts += torch.bincount(assign, minlength=counts.shape[0])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--dim", type=int, nargs="+", default=[192, 384, 768])
    ap.add_argument("--k", type=int, nargs="+", default=[64, 1024, 16384])
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="skip the fp16 route")
    ap.add_argument("--out", default=None, help="a JSON file of all results")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/kmeans_bench.py needs a HIP device: a time is a run on the GPU")
    results = []
    for rows in args.rows:
        for dim in args.dim:
            for K in args.k:
                x, cent = blobs(rows, dim, K, seed=rows + dim + K)
                km = cl.KMeans(K, dim, "cuda:0").set_centroids(cent)
                a, d = km.assign(x)
                km.stats.zero_()
                km.accumulate(x, a, d)
                torch.cuda.synchronize()
                n = min(rows, 64)                         # right before fast: the first rows against numpy, the totals against torch
                ra, rd = kmeans_assign_reference(x[:n].cpu().numpy(), cent.cpu().numpy())
                assert np.array_equal(a[:n].cpu().numpy(), ra) and np.array_equal(d[:n].cpu().numpy(), rd), (rows, dim, K)
                s, c, i = km.stats.numpy()
                assert c.sum() == rows and i == int(d.sum(dtype=torch.int64).item()) and np.array_equal(
                    s.sum(axis=0), x.sum(dim=0, dtype=torch.int64).cpu().numpy()), (rows, dim, K)
                keep = km.centroids.clone()
                t_assign, s1, r1 = timed(lambda: km.assign(x), args.window, args.repeat)
                t_acc, s2, r2 = timed(lambda: km.accumulate(x, a, d), args.window, args.repeat)
                t_upd, s3, r3 = timed(km.update, args.window, args.repeat)        # the same divisions every call, whatever the bytes were
                km.centroids.copy_(keep)
                ops = 2.0 * rows * K * dim
                res = {"rows": rows, "dim": dim, "K": K, "assign_ms": round(t_assign, 4), "assign_tops": round(ops / (t_assign * 1e-3) / 1e12, 2),
                       "assign_frac": round(ops / (t_assign * 1e-3) / 1e12 / INT8_PEAK_TOPS, 4), "acc_ms": round(t_acc, 4),
                       "acc_gbs": round(rows * dim * 8 / (t_acc * 1e-3) / 1e9, 1), "acc_form": "lds" if K * (dim + 1) * 4 <= 65536 else "global",
                       "update_ms": round(t_upd, 4), "assign_ms_range": s1, "acc_ms_range": s2, "update_ms_range": s3,
                       "reps": [r1, r2, r3]}
                if not args.no_torch:
                    sums = torch.zeros(K, dim, dtype=torch.float32, device="cuda")
                    counts = torch.zeros(K, dtype=torch.int64, device="cuda")
                    ta = torch_route(x, cent)
                    res["torch_agrees"] = round(float((ta == a.to(torch.int64)).float().mean().item()), 6)
                    t, res["torch_assign_ms_range"], _ = timed(lambda: torch_route(x, cent), args.window, args.repeat)
                    res["torch_assign_ms"] = round(t, 4)
                    t, res["torch_acc_ms_range"], _ = timed(lambda: torch_accumulate(x, ta, sums, counts), args.window, args.repeat)
                    res["torch_acc_ms"] = round(t, 4)
                    del sums, counts, ta
                results.append(res)
                print(json.dumps(res), flush=True)
                del x, cent, km, a, d
                torch.cuda.empty_cache()
    cols = ["rows", "dim", "K", "assign_ms", "assign_tops", "assign_frac", "acc_ms", "acc_gbs", "acc_form", "update_ms"] + (
        [] if args.no_torch else ["torch_assign_ms", "torch_acc_ms", "torch_agrees"])
    print("| " + " | ".join(cols) + " |")
    print("|" + "---|" * len(cols))
    for r in results:
        print("| " + " | ".join(
            "%s (%s – %s)" % (r[c], *r[c + "_range"]) if c + "_range" in r else str(r[c]) for c in cols) + " |")
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "int8_peak_tops": INT8_PEAK_TOPS, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
