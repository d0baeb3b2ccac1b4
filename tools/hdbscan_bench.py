"""Times HDBSCAN's device passes (include/ivit_hdbscan.h) on tools/density_bench.py's rows, beside the passes they were cut from —
`ivit_density_degree` and `ivit_linkage_round`, whose kernels this library leaves as they were — on the same box, INTERLEAVED.

    python tools/hdbscan_bench.py [--rows 100000] [--dim 384] [--centres 300] [--min-pts 5 16] [--out hdbscan_bench.json]

Reported per min_pts:
  core_ms, degree_ms, core_over_degree   ivit_core_similarity against ivit_density_degree (threshold 0.9): the same geometry, so the
                         ratio is the cost of the candidate lists (`--repeat` rounds, one window of each in turn; medians, [fastest,
                         slowest])
  reach_first_ms, linkage_first_ms, reach_over_linkage   ivit_linkage_init + the first ivit_reach_round against the same with
                         ivit_linkage_round, in the same interleaving
  hdbscan_forest_ms, linkage_forest_ms   the whole forests (`cluster.hdbscan`'s device part: core pass and rounds; and
                         `cluster.single_linkage`), the second run of each, with rounds and the peak device memory beyond the rows
  condense_ms, select_ms, clusters, noise_share   the host part over the forest's edges
The device results are compared with `predict.hdbscan_reference` on the first 1024 rows before anything is timed.  The saturation exit
of the reach scan is timed on and off by running this tool twice, the second time with IVIT_LIB naming a library built without it
(`library` in the output says which one ran).  Prints one JSON line; needs a HIP device."""
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
from ivit_amd.predict import hdbscan_reference, inv_norms_reference  # noqa: E402
from density_bench import clustered_rows, timed  # noqa: E402
from range_bench import P, interleaved, inv_norms  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--centres", type=int, default=300)
    ap.add_argument("--min-pts", type=int, nargs="+", default=[5, 16])
    ap.add_argument("--min-cluster-size", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.15)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/hdbscan_bench.py needs a HIP device: a time is a run on the GPU")
    h = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    rows, dim = args.rows, args.dim
    x = clustered_rows(rows, dim, args.centres, rows + dim)
    w = inv_norms(h, x)
    small = x[:1024].contiguous()
    ref = hdbscan_reference(small.cpu().numpy(), inv_norms_reference(small.cpu().numpy()), args.min_pts[0])
    _, core, tree, _ = cluster.hdbscan(small, args.min_cluster_size, args.min_pts[0])
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip((core, tree.u, tree.v, tree.val), ref)), "the device differs from hdbscan_reference"

    n, nd = ctypes.c_size_t(), ctypes.c_size_t()
    h.call("ivit_density_workspace_bytes", rows, dim, 0, ctypes.byref(nd))
    h.call("ivit_linkage_workspace_bytes", rows, dim, 0, ctypes.byref(n))
    new = lambda dt, m=rows: torch.empty(m, dtype=dt, device="cuda")      # noqa: E731
    dws, degree, ws, core = new(torch.uint8, nd.value), new(torch.int32), new(torch.uint8, n.value), new(torch.float32)
    comp, done, u, v, val, state = new(torch.int32), new(torch.uint8), new(torch.int32), new(torch.int32), new(torch.float32), new(torch.int32, 4)
    run = tuple(P(t) for t in (comp, done, u, v, val, state))
    res = {"rows": rows, "dim": dim, "library": _lib.SO_PATH, "linkage_forest": {}}
    for min_pts in args.min_pts:
        nc = ctypes.c_size_t()
        h.call("ivit_core_workspace_bytes", rows, dim, min_pts, 0, ctypes.byref(nc))
        cws = new(torch.uint8, nc.value)
        core_pass = lambda: h.call("ivit_core_similarity", P(x), rows, dim, P(w), min_pts, 0, P(cws), nc.value, P(core))      # noqa: E731
        core_pass()

        def reach_first():
            h.call("ivit_linkage_init", rows, *run)
            h.call("ivit_reach_round", P(x), rows, dim, P(w), P(core), float("-inf"), 0, P(ws), n.value, *run)

        def linkage_first():
            h.call("ivit_linkage_init", rows, *run)
            h.call("ivit_linkage_round", P(x), rows, dim, P(w), float("-inf"), 0, P(ws), n.value, *run)
        t = interleaved({"core": core_pass, "reach_first": reach_first, "linkage_first": linkage_first,
                         "degree": lambda: h.call("ivit_density_degree", P(x), rows, dim, P(w), 0.9, 0, P(dws), nd.value, P(degree))},
                        args.window, args.repeat)
        r = {name + "_ms": round(t[name][0], 4) for name in t}
        r.update({name + "_ms_range": t[name][1] for name in t})
        r.update(core_over_degree=round(t["core"][0] / t["degree"][0], 4), reach_over_linkage=round(t["reach_first"][0] / t["linkage_first"][0], 4))
        del cws
        device_part = lambda: cluster._forest(h, x, rows, dim, w, None, 0, 1, cluster._core(h, x, rows, dim, w, min_pts, 0))      # noqa: E731
        forest, ms, peak = timed(device_part)
        forest, ms, peak = timed(device_part)                           # the second run: warm
        r.update(hdbscan_forest_ms=round(ms, 3), hdbscan_forest_peak_bytes=int(peak), rounds=forest.rounds, edges=int(forest.u.shape[0]))
        t0 = time.perf_counter()
        condensed = forest.condense(args.min_cluster_size)
        t1 = time.perf_counter()
        label = condensed.select()
        r.update(condense_ms=round((t1 - t0) * 1e3, 1), select_ms=round((time.perf_counter() - t1) * 1e3, 1), clusters=int(len(np.unique(label[label >= 0]))),
                 noise_share=round(float((label < 0).mean()), 4))
        res["min_pts_%d" % min_pts] = r
    tree, ms, peak = timed(lambda: cluster.single_linkage(x))
    tree, ms, peak = timed(lambda: cluster.single_linkage(x))
    res["linkage_forest"] = {"ms": round(ms, 3), "peak_bytes": int(peak), "rounds": tree.rounds}
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "result": res}, f, indent=1)


if __name__ == "__main__":
    main()
