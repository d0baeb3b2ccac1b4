"""Novelty scores (include/ivit_gauss.h), timed beside the plain torch route, and the two routes' errors against float64.

    python tools/gauss_bench.py                       # 100 000 x 384 and 256 x 384, R = 384, C = 1000: one JSON line of times each
    python tools/gauss_bench.py --errors              # the test shapes, then every width of tests/float_cases.py: the largest error
                                                      # of each route against gauss_score_reference, per list; the one-hot models

The torch route is what a user writes without the entry: z = feat8.float() @ Wh.T + t, q = (z * z).sum(1), s = feat8.float() @ Wc.T +
bc, max — fp32, its [N, R] and [N, C] matrices materialised.  Times: device events round `--reps` calls, the routes alternating in
`--rounds` rounds after a warm-up of all; the median round of each is reported with the smallest and largest.  `prepare` is one
ivit_gauss_prepare of the model (once per model, not per batch).  One device."""
import argparse
import json
import os
import sys

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, "tests"))
import float_cases  # noqa: E402    the generator and the case lists the tests bound (tests/float_cases.py)
from ivit_amd import gauss  # noqa: E402
from ivit_amd.predict import gauss_score_reference  # noqa: E402

# tests/test_gauss_gpu.py: SHAPES
SHAPES = [(1, 64, 32, 1, 3), (127, 192, 96, 33, 1), (129, 64, 64, 70, 0), (300, 192, 192, 70, 3), (300, 1024, 96, 33, 0), (129, 1024, 1024, 1, 1),
          (127, 64, 32, 70, 0), (300, 1024, 32, 70, 3), (1, 192, 32, 33, 1), (129, 128, 128, 33, 3), (300, 128, 96, 1, 0), (127, 192, 192, 1, 3),
          (129, 448, 96, 70, 0), (300, 512, 512, 33, 1)]


def case(N, dim, R, C, seed=0):
    x, *model = float_cases.gauss_arrays(N, dim, R, C, seed)
    return x, gauss.GaussModel(*model)


def torch_route(x8, Wh, t, Wc, bc):
    x = x8.float()
    z = x @ Wh.T + t
    q = (z * z).sum(dim=1)
    best, cls = (x @ Wc.T + bc).max(dim=1)
    return q - best, cls, q, best


def errors(got, x, m):
    """(|q - q64| / max q64, |best - best64| / max |s64|), the largest over the rows"""
    _, _, q, best = gauss_score_reference(x, m.Wh, m.t, m.Wc, m.bc)
    smax = np.abs(x.astype(np.float64) @ m.Wc.astype(np.float64).T + m.bc.astype(np.float64)).max()
    return float(np.abs(got[2] - q).max() / q.max()), float(np.abs(got[3] - best).max() / smax)


def time_routes(routes, reps, rounds):
    for f in routes.values():
        for _ in range(3):
            f()
    times = {k: [] for k in routes}
    for _ in range(rounds):
        for k, f in routes.items():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                f()
            e.record()
            e.synchronize()
            times[k].append(a.elapsed_time(e) / reps)
    return {k + "_ms": {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)} for k, t in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--errors", action="store_true")
    ap.add_argument("--n", type=int, nargs="+", default=[100000, 256])
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--rank", type=int, default=384)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--splits", type=int, default=0)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/gauss_bench.py needs a HIP device")
    if args.errors:
        for name, shapes in (("the test shapes", [s + (0,) for s in SHAPES]), ("every width", float_cases.GAUSS_WIDTH_CASES)):
            worst = {"torch": [0.0, 0.0], "entry": [0.0, 0.0]}
            for N, dim, R, C, splits, seed in shapes:
                x, m = case(N, dim, R, C, seed)
                xd = torch.from_numpy(x).cuda()
                dev = [torch.from_numpy(a).cuda() for a in (m.Wh, m.t, m.Wc, m.bc)]
                rows = {"torch": errors([t.cpu().numpy() for t in torch_route(xd, *dev)], x, m),
                        "entry": errors([t.cpu().numpy() for t in gauss.score(xd, m, splits)], x, m)}
                for k, e in rows.items():
                    worst[k] = [max(a, c) for a, c in zip(worst[k], e)]
                print(json.dumps({"case": [N, dim, R, C, splits], **{k: ["%.3e" % v for v in e] for k, e in rows.items()}}), flush=True)
            print(json.dumps({"list": name, "worst (q, best)": {k: ["%.3e" % v for v in e] for k, e in worst.items()}}), flush=True)
        # the one-hot models have no tolerance: the number of elements of each output that differ from the expectation in any bit
        for dim, R, splits in float_cases.ONEHOT_GAUSS_CASES:
            x, *model = float_cases.onehot_case(dim, R)
            want = float_cases.onehot_gauss_expected(x, *model)
            got = gauss.score(torch.from_numpy(np.array(x)).cuda(), gauss.GaussModel(*(np.array(a) for a in model)), splits)    # copies: read-only arrays
            print(json.dumps({"one-hot": [dim, R, splits], "differing (dist, cls, q, best)":
                              [int((g.cpu().numpy().view(np.uint32) != w.view(np.uint32)).sum()) for g, w in zip(got, want)]}), flush=True)
        return
    for n in args.n:
        x, m = case(n, args.dim, args.rank, args.classes)
        xd = torch.from_numpy(x).cuda()
        dev = [torch.from_numpy(a).cuda() for a in (m.Wh, m.t, m.Wc, m.bc)]
        h, model = m.prepared(xd.device)
        P = lambda t: gauss._P(t.data_ptr())
        routes = {"entry": lambda: gauss.score(xd, m, args.splits), "torch": lambda: torch_route(xd, *dev),
                  "prepare": lambda: h.call("ivit_gauss_prepare", *(P(a) for a in dev), m.dim, m.R, m.C, P(model), model.numel())}
        got, ref = routes["entry"](), routes["torch"]()
        agree = float((got[2] - ref[2]).abs().max() / ref[2].abs().max())
        print(json.dumps({"n": n, "dim": args.dim, "rank": args.rank, "classes": args.classes, "splits": args.splits, "reps": args.reps,
                          "rounds": args.rounds, "q entry vs torch, rel. to max": "%.2e" % agree, **time_routes(routes, args.reps, args.rounds)}))


if __name__ == "__main__":
    main()
