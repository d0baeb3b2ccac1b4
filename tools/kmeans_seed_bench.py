"""Times the device k-means++ seeding (include/ivit_seed.h) beside the host seeding it stands in for, on one box in one session.

    python tools/kmeans_seed_bench.py [--rows 65536] [--big-rows 1048576] [--dim 384] [--k 256 1024] [--repeat 5] [--out seed_bench.json]

Seeded blobs (tools/kmeans_bench.py's).  Every device time is a host clock round one `cluster.seed` call that ends in a device
synchronise, after a warm-up of the same shape: the median of --repeat calls with [fastest, slowest] beside it; device and host runs
alternate.  Reported, one JSON line each:
  host_vs_device   per K at --rows x --dim: device_ms at trials 1 and at the default, host_ms (`cluster.init_centroids` on the rows
                   already in host memory: the copy is not counted; --host-repeat runs) and the ratios
  big              the device seeding alone at --big-rows, K = the largest --k, default trials; per_centre_us is the slope between that
                   K and a quarter of it (three launches: scan, pick, locate) and stream_gbs the bytes of x over it — a LOWER bound of
                   the scan's own rate, which has no entry of its own; copy_gbs is a device-to-device copy of the same bytes (read
                   + write counted once, as bytes copied) timed with device events
  inertia          the first-iteration inertia of `fit` from "sample", host "kmeans++" and the device greedy seeds on the same rows
The device result is compared with `predict.kmeans_seed_reference` at 4096 rows before anything is timed.  Needs a HIP device."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ivit_amd  # noqa: E402,F401
from ivit_amd import cluster as cl  # noqa: E402
from ivit_amd.predict import kmeans_seed_reference  # noqa: E402
from kmeans_bench import blobs  # noqa: E402


def wall(fn, repeat):
    """(median ms, [min, max]) of fn() + synchronise over `repeat` runs, after one warm-up"""
    out = []
    for i in range(repeat + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    out = out[1:]
    return round(statistics.median(out), 3), [round(min(out), 3), round(max(out), 3)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--big-rows", type=int, default=1048576)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--k", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--host-repeat", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/kmeans_seed_bench.py needs a HIP device: a time is a run on the GPU")
    results = []

    def emit(r):
        results.append(r)
        print(json.dumps(r), flush=True)

    x, _ = blobs(4096, args.dim, 64, seed=1)                      # right before fast
    first, draws = cl.seed_draws(4096, 64, cl.default_trials(64), np.random.default_rng(0))
    want = kmeans_seed_reference(x.cpu().numpy(), 64, first, draws)
    got = cl.seed(x, 64)
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[2].cpu().numpy(), want[3])

    x, _ = blobs(args.rows, args.dim, max(args.k), seed=2)
    xh = x.cpu().numpy()
    for K in args.k:
        r = {"what": "host_vs_device", "rows": args.rows, "dim": args.dim, "K": K, "default_trials": cl.default_trials(K)}
        for name, trials in (("device_ms_trials1", 1), ("device_ms_default", None)):
            r[name], r[name + "_range"] = wall(lambda: cl.seed(x, K, trials=trials), args.repeat)
        host = []
        for _ in range(args.host_repeat):                         # between device runs of the next K: alternating
            t0 = time.perf_counter()
            cl.init_centroids(xh, K, "kmeans++", np.random.default_rng(0), init_rows=args.rows)
            host.append((time.perf_counter() - t0) * 1e3)
        r["host_ms"], r["host_ms_range"] = round(statistics.median(host), 1), [round(min(host), 1), round(max(host), 1)]
        r["host_over_device_trials1"] = round(r["host_ms"] / r["device_ms_trials1"], 1)
        r["host_over_device_default"] = round(r["host_ms"] / r["device_ms_default"], 1)
        emit(r)

    K = args.k[0]                                                 # the quality the trials buy: one Lloyd iteration from each seeding
    r = {"what": "inertia", "rows": args.rows, "dim": args.dim, "K": K}
    for name, kw in (("sample", dict(method="sample")), ("host_kmeans++", dict(method="kmeans++", init_rows=args.rows)),
                     ("device_trials1", dict(where="device", trials=1)), ("device_greedy", dict(where="device"))):
        km = cl.KMeans(K, args.dim, "cuda:0").init(xh if "where" not in kw else x, generator=np.random.default_rng(0), **kw)
        r[name] = int(km.fit(x, iters=1)[0])
    emit(r)
    del x, xh

    K = max(args.k)
    x, _ = blobs(args.big_rows, args.dim, K, seed=3)
    r = {"what": "big", "rows": args.big_rows, "dim": args.dim, "K": K, "trials": cl.default_trials(K)}
    r["device_ms"], r["device_ms_range"] = wall(lambda: cl.seed(x, K, trials=r["trials"]), args.repeat)
    r["device_ms_quarter_K"], _ = wall(lambda: cl.seed(x, K // 4, trials=r["trials"]), args.repeat)
    r["per_centre_us"] = round((r["device_ms"] - r["device_ms_quarter_K"]) / (K - K // 4) * 1e3, 2)
    r["stream_gbs"] = round(x.numel() / (r["per_centre_us"] * 1e-6) / 1e9, 1)
    y, times = torch.empty_like(x), []
    for i in range(args.repeat + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            y.copy_(x)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / 20)
    r["copy_ms"] = round(statistics.median(times[1:]), 4)
    r["copy_gbs"] = round(x.numel() / (r["copy_ms"] * 1e-3) / 1e9, 1)
    emit(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
