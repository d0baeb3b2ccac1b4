"""One loss / gradient evaluation of the logistic probe, timed beside the plain torch route, and the two routes' errors against float64.

    python tools/logreg_bench.py                      # N = 100 000, dim = 384, C = 1000: one JSON line of times
    python tools/logreg_bench.py --errors             # the test shapes, then the case lists of tests/float_cases.py: the largest
                                                      # error of each route against logreg_reference, per list

The torch route is what a user writes without the entry: z = (feat8.float() @ W.T) * x_scale + b, log-softmax, p - onehot, two
matmuls in fp32; its [N, C] matrices are materialised.  Times: device events round `--reps` evaluations, the two routes alternating
in `--rounds` rounds after a warm-up of both; the median round of each is reported with the smallest and largest.  One device."""
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
from ivit_amd.predict import logreg_reference  # noqa: E402
from ivit_amd.probe import logreg_loss_grad  # noqa: E402

# tests/test_logreg_gpu.py: SHAPES and (in test_cases) its two further cases under the accuracy rule
SHAPES = [(1, 2, 64, 0), (127, 2, 192, 1), (129, 33, 64, 3), (300, 70, 192, 0), (300, 33, 1024, 1), (129, 70, 1024, 3), (127, 70, 64, 0),
          (300, 2, 1024, 3), (1, 33, 192, 1), (129, 2, 64, 1), (300, 70, 64, 3), (127, 33, 192, 0)]
case = float_cases.logreg_case


def torch_route(x8, lab, W, b, s):
    x = x8.float()
    z = (x @ W.T) * s + b
    keep = (lab >= 0) & (lab < W.shape[0])               # a row outside the range counts for nothing
    at = lab.long().clamp(0, W.shape[0] - 1)
    lse = torch.logsumexp(z, dim=1)
    loss = ((lse - z.gather(1, at[:, None])[:, 0]) * keep).sum()
    g = torch.exp(z - lse[:, None])
    g[torch.arange(len(lab), device=g.device), at] -= 1.0
    g = g * keep[:, None]
    return loss, g.T @ x, g.sum(dim=0)


def test_cases():
    """(name, x, labels, W, b, x_scale, splits): every case tests/test_logreg_gpu.py holds to the accuracy rule"""
    for N, C, dim, splits in SHAPES:
        yield ([N, C, dim, splits],) + case(N, C, dim) + (splits,)
    x, lab, W, b, s = case(300, 33, 192, seed=1)
    lab[::3] = np.array([-1, 33, 2 ** 31 - 1, -2 ** 31])[np.arange(100) % 4]
    yield ("labels outside the range", x, lab, W, b, s, 0)
    x, lab, W, b, s = case(129, 33, 192, seed=2)
    x[7] = -128
    W[0], W[1] = 80 / (s * 128 * 192), -80 / (s * 128 * 192)
    b[:2] = 0
    yield ("logits of +-80", x, lab, W, b, s, 1)


def further_lists():
    """(list name, its cases in test_cases' form): the case lists of tests/float_cases.py, each with constants of its own"""
    yield "every width", [([N, C, dim, splits],) + case(N, C, dim, seed) + (splits,) for N, C, dim, splits, seed in float_cases.LOGREG_WIDTH_CASES]
    yield "both sides of LOGREG_FLUSH_ROWS", [([N, C, dim, splits],) + case(N, C, dim, seed) + (splits,)
                                              for N, C, dim, splits, seed in float_cases.LOGREG_FLUSH_CASES]
    yield "one-hot models", [(["one-hot", dim, splits],) + float_cases.onehot_logreg_case(dim) + (splits,) for dim, splits in float_cases.ONEHOT_LOGREG_CASES]


def walk(name, cases):
    worst = {"torch": [0.0, 0.0, 0.0], "entry": [0.0, 0.0, 0.0]}
    for label, x, lab, W, b, s, splits in cases:
        want = logreg_reference(x, lab, W, b, s)
        dev = [torch.from_numpy(np.array(a)).cuda() for a in (x, lab, W, b)]      # a copy: the one-hot arrays are read-only
        rows = {"torch": errors([t.cpu().numpy() for t in torch_route(*dev, s)], want),
                "entry": errors([t.cpu().numpy() for t in logreg_loss_grad(*dev, s, splits)[:3]], want)}
        for k, e in rows.items():
            worst[k] = [max(a, c) for a, c in zip(worst[k], e)]
        print(json.dumps({"case": label, **{k: ["%.3e" % v for v in e] for k, e in rows.items()}}), flush=True)
    print(json.dumps({"list": name, "worst (loss, grad_W, grad_b)": {k: ["%.3e" % v for v in e] for k, e in worst.items()}}), flush=True)


def errors(got, want):
    return (abs(float(np.asarray(got[0]).reshape(-1)[0]) - want[0]) / abs(want[0]), float(np.abs(got[1] - want[1]).max() / np.abs(want[1]).max()),
            float(np.abs(got[2] - want[2]).max() / np.abs(want[2]).max()))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--errors", action="store_true")
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--splits", type=int, default=0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/logreg_bench.py needs a HIP device")
    if args.errors:
        walk("the test shapes", test_cases())
        for name, cases in further_lists():
            walk(name, cases)
        return
    x, lab, W, b, s = case(args.n, args.classes, args.dim)
    dev = [torch.from_numpy(a).cuda() for a in (x, lab, W, b)]
    routes = {"entry": lambda: logreg_loss_grad(*dev, s, args.splits), "torch": lambda: torch_route(*dev, s)}
    got, ref = routes["entry"](), routes["torch"]()
    agree = float((got[1] - ref[1]).abs().max() / ref[1].abs().max())
    for f in routes.values():
        for _ in range(3):
            f()
    times = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, f in routes.items():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                f()
            e.record()
            e.synchronize()
            times[k].append(a.elapsed_time(e) / args.reps)
    print(json.dumps({"n": args.n, "dim": args.dim, "classes": args.classes, "splits": args.splits, "reps": args.reps, "rounds": args.rounds,
                      "grad_W entry vs torch, rel. to max": "%.2e" % agree,
                      **{k + "_ms": {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)} for k, t in times.items()}}))


if __name__ == "__main__":
    main()
