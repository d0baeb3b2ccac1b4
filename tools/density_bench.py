"""Times the density clustering (include/ivit_density.h) beside the route a user has without it — `Gallery.within` with the triangle
(the pair list of include/ivit_range.h) and `search.duplicate_groups` on the host — on the same box, INTERLEAVED.

    python tools/density_bench.py [--rows 100000] [--dim 384] [--centres 300] [--neighbours 300] [--min-pts 5] [--out density_bench.json]

The rows are random-clustered: --centres random int8 centres, every row a centre plus noise; the cosine threshold is read from the
scores of a sample so that a row has about --neighbours neighbours.  Reported:
  degree_ms, range_count_ms, degree_over_range_count   the degree pass against ivit_range_count on the same self-join without the
                         triangle: the same MFMA work (`--repeat` rounds, every round one window of each in turn; medians, [fastest,
                         slowest] beside them)
  sweeps, skipped_share  the sweeps until `changed` is 0, stepped one at a time, and per sweep the share of tiles dirty_in does not mark
  dbscan_ms              `cluster.dbscan` at min_pts (check_every 4), everything included; dbscan_peak_bytes beside it
  pairs_ms               `Gallery.within(triangle)` + `duplicate_groups`, the same components at min_pts = 1, pairs_peak_bytes and the
                         number of pairs beside it; if the pair list does not fit in --pair-limit bytes (from ivit_range_count's total,
                         before anything is allocated) the route is not run and the bytes it would need are reported: that is the
                         point of the feature
The device labels are compared with `predict.dbscan_reference` on the first 2048 rows before anything is timed.  Prints one JSON line;
needs a HIP device."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ivit_amd  # noqa: E402,F401
from ivit_amd import _lib, cluster  # noqa: E402
from ivit_amd.predict import dbscan_reference, inv_norms_reference  # noqa: E402
from ivit_amd.search import Gallery, duplicate_groups  # noqa: E402
from range_bench import P, interleaved, inv_norms  # noqa: E402


def clustered_rows(n, dim, centres, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    c = torch.randint(-60, 61, (centres, dim), generator=g, device="cuda", dtype=torch.int32)
    pick = torch.randint(0, centres, (n,), generator=g, device="cuda")
    noise = torch.randint(-40, 41, (n, dim), generator=g, device="cuda", dtype=torch.int32)
    return (c[pick] + noise).clamp(-128, 127).to(torch.int8).contiguous()


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--centres", type=int, default=300)
    ap.add_argument("--neighbours", type=int, default=300)
    ap.add_argument("--min-pts", type=int, default=5)
    ap.add_argument("--pair-limit", type=float, default=8e9, help="bytes of pair list above which the existing route is not run")
    ap.add_argument("--window", type=float, default=0.15)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/density_bench.py needs a HIP device: a time is a run on the GPU")
    h = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    rows, dim = args.rows, args.dim
    x = clustered_rows(rows, dim, args.centres, rows + dim)
    w = inv_norms(h, x)
    sample = (x[:256].float() @ x[:65536].float().T) * w[:65536][None, :] * w[:256, None]
    thr = float(torch.quantile(sample.flatten()[:1 << 22], 1 - args.neighbours / rows).item())
    del sample

    small = x[:2048].contiguous()
    got = cluster.dbscan(small, thr, args.min_pts)
    ref = dbscan_reference(small.cpu().numpy(), inv_norms_reference(small.cpu().numpy()), thr, args.min_pts)
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got[:3], ref)), "the device differs from dbscan_reference"

    n = ctypes.c_size_t()
    h.call("ivit_density_workspace_bytes", rows, dim, 0, ctypes.byref(n))
    ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    scan = (P(x), rows, dim, P(w), thr, 0, P(ws), n.value)
    degree = torch.empty(rows, dtype=torch.int32, device="cuda")
    h.call("ivit_range_workspace_bytes", rows, rows, dim, 0, ctypes.byref(n))
    rws = torch.empty(max(n.value, 8), dtype=torch.uint8, device="cuda")
    row_ptr = torch.empty(rows + 1, dtype=torch.int64, device="cuda")
    t = interleaved({"degree": lambda: h.call("ivit_density_degree", *scan, P(degree)),
                     "range_count": lambda: h.call("ivit_range_count", P(x), rows, P(x), rows, dim, P(w), P(w), thr, 0, 0, 0, 0, P(rws), rws.numel(),
                                                   P(row_ptr))}, args.window, args.repeat)
    # ivit_range_count multiplies by the gallery row's weight first whichever row is larger: where the two roundings differ in the last
    # bit at the threshold its rows are not symmetric, and a count may differ from the degree by the pairs concerned
    differ = int((degree.to(torch.int64) != row_ptr[1:] - row_ptr[:-1]).sum().item())
    res = {"rows": rows, "dim": dim, "threshold": thr, "min_pts": args.min_pts, "mean_degree": float(degree.float().mean().item()),
           "degree_ms": round(t["degree"][0], 4), "degree_ms_range": t["degree"][1], "range_count_ms": round(t["range_count"][0], 4),
           "range_count_ms_range": t["range_count"][1], "degree_over_range_count": round(t["degree"][0] / t["range_count"][0], 4), "rows_where_range_count_differs": differ}
    del rws, row_ptr

    # the sweeps one at a time: how many, and what share of the tiles each skips
    tiles = (rows + 31) // 32
    words = (tiles + 63) // 64
    label = [torch.empty(rows, dtype=torch.int32, device="cuda") for _ in range(2)]
    dirty = [torch.empty(words, dtype=torch.int64, device="cuda") for _ in range(2)]
    changed = torch.empty(1, dtype=torch.int32, device="cuda")
    h.call("ivit_density_init", P(degree), rows, args.min_pts, P(label[0]), P(dirty[0]))
    skipped, sweep_ms, k = [], [], 0
    while True:
        marked = int(sum(bin(int(v) & (2 ** 64 - 1)).count("1") for v in dirty[k & 1].cpu().tolist()))
        skipped.append(round(1 - marked / tiles, 4))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        h.call("ivit_density_sweep", *scan, P(label[k & 1]), P(dirty[k & 1]), P(label[~k & 1]), P(dirty[~k & 1]), P(changed))
        b.record()
        torch.cuda.synchronize()
        sweep_ms.append(round(a.elapsed_time(b), 4))
        k += 1
        if int(changed.item()) == 0:
            break
    res.update(sweeps=k, skipped_share=skipped, sweep_ms=sweep_ms)
    del label, dirty, ws, degree

    out, ms, peak = timed(lambda: cluster.dbscan(x, thr, args.min_pts))
    out, ms, peak = timed(lambda: cluster.dbscan(x, thr, args.min_pts))               # the second run: warm
    label = out[0]
    res.update(dbscan_ms=round(ms, 3), dbscan_peak_bytes=int(peak), dbscan_sweeps=out[3], clusters=int(cluster.compact_labels(label)[1]),
               noise_share=float((label < 0).float().mean().item()))
    groups, gms, gpeak = timed(lambda: cluster.dbscan(x, thr, 1))
    pairs = int((res["mean_degree"] - 1) * rows / 2)
    need = pairs * (4 + 4 + 16)                                                       # idx, val, and the int64 [P, 2] pairs
    res.update(groups_ms=round(gms, 3), groups_peak_bytes=int(gpeak), pairs=pairs)
    if need > args.pair_limit:
        res.update(pairs_route="not run: the pair list does not fit", pairs_bytes_needed=need)
    else:
        gal = Gallery(x, cosine=True)

        def route():
            row_ptr, idx, _ = gal.within(x, thr, triangle=True)
            i = torch.repeat_interleave(torch.arange(rows, device="cuda"), row_ptr[1:] - row_ptr[:-1])
            return duplicate_groups(torch.stack([i, idx.to(torch.int64)], 1), rows)
        want, pms, ppeak = timed(route)
        g = groups[0].cpu().numpy().astype(np.int64)
        assert np.array_equal(np.where(g < 0, np.arange(rows), g), want), "the two routes differ"
        res.update(pairs_ms=round(pms, 3), pairs_peak_bytes=int(ppeak))
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "result": res}, f, indent=1)


if __name__ == "__main__":
    main()
