"""Times the single-linkage hierarchy (include/ivit_linkage.h) on tools/density_bench.py's rows, beside the degree pass of
include/ivit_density.h — the same MFMA work as one round's scan — on the same box, INTERLEAVED.

    python tools/linkage_bench.py [--rows 100000] [--dim 384] [--centres 300] [--floor 0.9] [--out linkage_bench.json]

Reported:
  first_round_ms, degree_ms, round_over_degree   ivit_linkage_init + the first ivit_linkage_round (every row its own component: the
                         scan with nothing skipped, and the five small launches behind it) against ivit_density_degree at the floor
                         as threshold (`--repeat` rounds, every round one window of each in turn; medians, [fastest, slowest])
  round_ms, components, early_share   a whole run stepped one round at a time: the time of every round, the components before it and
                         the share of wavefronts (32 rows) all of whose rows belong to done components, which leave without a walk
  linkage_ms, linkage_floor_ms   `cluster.single_linkage` with floor None and with --floor, everything included (the second run of
                         each), rounds, edges and the peak device memory beyond the rows beside them
  dbscan_ms              `cluster.dbscan(min_pts=1)` at --floor: ONE point of the threshold sweep the tree replaces
The device tree is compared with `predict.linkage_reference` on the first 1024 rows before anything is timed, and its cut at --floor
with the dbscan groups after.  Prints one JSON line; needs a HIP device."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ivit_amd  # noqa: E402,F401
from ivit_amd import _lib, cluster  # noqa: E402
from ivit_amd.predict import inv_norms_reference, linkage_reference  # noqa: E402
from density_bench import clustered_rows, timed  # noqa: E402
from range_bench import P, interleaved, inv_norms  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--centres", type=int, default=300)
    ap.add_argument("--floor", type=float, default=0.9)
    ap.add_argument("--window", type=float, default=0.15)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/linkage_bench.py needs a HIP device: a time is a run on the GPU")
    h = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    rows, dim = args.rows, args.dim
    x = clustered_rows(rows, dim, args.centres, rows + dim)
    w = inv_norms(h, x)

    small = x[:1024].contiguous()
    got, ref = cluster.single_linkage(small), linkage_reference(small.cpu().numpy(), inv_norms_reference(small.cpu().numpy()))
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip((got.u, got.v, got.val), ref)), "the device differs from linkage_reference"

    n = ctypes.c_size_t()
    h.call("ivit_density_workspace_bytes", rows, dim, 0, ctypes.byref(n))
    dws, degree = torch.empty(n.value, dtype=torch.uint8, device="cuda"), torch.empty(rows, dtype=torch.int32, device="cuda")
    h.call("ivit_linkage_workspace_bytes", rows, dim, 0, ctypes.byref(n))
    ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    new = lambda dt, m=rows: torch.empty(m, dtype=dt, device="cuda")      # noqa: E731
    comp, done, u, v, val, state = new(torch.int32), new(torch.uint8), new(torch.int32), new(torch.int32), new(torch.float32), new(torch.int32, 4)
    run = tuple(P(t) for t in (comp, done, u, v, val, state))
    round_ = lambda floor: h.call("ivit_linkage_round", P(x), rows, dim, P(w), floor, 0, P(ws), n.value, *run)      # noqa: E731

    def first_round():
        h.call("ivit_linkage_init", rows, *run)
        round_(float("-inf"))
    t = interleaved({"first_round": first_round,
                     "degree": lambda: h.call("ivit_density_degree", P(x), rows, dim, P(w), args.floor, 0, P(dws), dws.numel(), P(degree))},
                    args.window, args.repeat)
    res = {"rows": rows, "dim": dim, "floor": args.floor, "first_round_ms": round(t["first_round"][0], 4), "first_round_ms_range": t["first_round"][1],
           "degree_ms": round(t["degree"][0], 4), "degree_ms_range": t["degree"][1], "round_over_degree": round(t["first_round"][0] / t["degree"][0], 4)}
    del dws, degree

    for name, floor in (("rounds_none", float("-inf")), ("rounds_floor", args.floor)):
        h.call("ivit_linkage_init", rows, *run)
        ms, comps, early = [], [], []
        while True:
            components, merged = state.tolist()[:2]
            if merged == 0 or components == 1:
                break
            idle = torch.nn.functional.pad(done[comp.long()], (0, -rows % 32), value=1).view(-1, 32).bool().all(dim=1)
            comps.append(components)
            early.append(round(float(idle.float().mean().item()), 4))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            round_(floor)
            b.record()
            torch.cuda.synchronize()
            ms.append(round(a.elapsed_time(b), 4))
        res[name] = {"round_ms": ms, "components": comps, "early_share": early, "left": state.tolist()[0]}
    del ws, comp, done, u, v, val

    for name, floor in (("linkage", None), ("linkage_floor", args.floor)):
        tree, ms, peak = timed(lambda: cluster.single_linkage(x, floor=floor))
        tree, ms, peak = timed(lambda: cluster.single_linkage(x, floor=floor))      # the second run: warm
        res.update({name + "_ms": round(ms, 3), name + "_peak_bytes": int(peak), name + "_rounds": tree.rounds, name + "_edges": int(tree.u.shape[0])})
    out, ms, peak = timed(lambda: cluster.dbscan(x, args.floor, 1))
    out, ms, peak = timed(lambda: cluster.dbscan(x, args.floor, 1))
    g = out[0].cpu().numpy().astype(np.int64)
    assert np.array_equal(np.where(g < 0, np.arange(rows), g), tree.cut(args.floor)), "the cut of the tree differs from the dbscan groups"
    res.update(dbscan_ms=round(ms, 3), dbscan_peak_bytes=int(peak), dbscan_sweeps=out[3], groups=int(len(np.unique(g[g >= 0])) + (g < 0).sum()))
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "result": res}, f, indent=1)


if __name__ == "__main__":
    main()
