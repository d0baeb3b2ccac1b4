"""Times the two passes of the range search (include/ivit_range.h) and, beside them on the same box and INTERLEAVED with them,
ivit_search_topk at k = 1 — the same single pass over the same gallery, per score what the count pass does plus the key
bookkeeping — and, on the smallest shape only, the route a user has without the entries: ivit_linear_i8 to the [queries, gallery]
int32 matrix, then torch.nonzero.

    python tools/range_bench.py [--dim 384 768] [--rows 131072 1048576] [--nq 256] [--self-join 131072] [--out range_bench.json]

Per (rows, dim) on seeded int8 rows with the gallery's inverse norms as weights, at three thresholds read from the scores of a
sample so that about 0, 1e-4 and 1e-2 of the scores hit: `--repeat` rounds, every round ONE window of each entry in turn (count,
fill, top-k; device events around `reps` back-to-back calls, reps sized so that a window lasts about --window seconds); the median
over the rounds with [fastest, slowest] window beside it.  Reported: count_ms, fill_ms, topk1_ms, count_over_topk1 (the ratio the
count pass is judged by), hits_per_score as measured, and for the smallest shape matrix_ms.  The self-join (--self-join N rows
against themselves, dim the first of --dim): the count and fill passes with and without the triangle, their ratio and beside it the
ratio of 32 x 32 tiles a wavefront loads that predicts it.  The device result is compared with `predict.range_reference` on the
first 64 queries and 4096 rows before anything is timed.  Prints one JSON line per case; needs a HIP device."""
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
from ivit_amd import _lib  # noqa: E402
from ivit_amd.predict import range_reference  # noqa: E402

_P = ctypes.c_void_p


def P(t):
    return None if t is None else _P(t.data_ptr())


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def interleaved(fns, seconds, repeat):
    """{name: (median ms, [fastest, slowest])}: `repeat` rounds, every round one window of every fn in turn"""
    reps = {}
    for name, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        reps[name] = int(max(3, seconds / max(time.perf_counter() - t0, 1e-6)))
    out = {name: [] for name in fns}
    for _ in range(repeat):
        for name, fn in fns.items():
            out[name].append(window(fn, reps[name]))
    return {name: (statistics.median(v), [round(min(v), 4), round(max(v), 4)]) for name, v in out.items()}


class Range:
    """the buffers and the two calls of one (queries, gallery, threshold)"""

    def __init__(self, h, q, g, w, qw, thr, triangle=False):
        self.h, (self.nq, self.dim), self.rows = h, q.shape, g.shape[0]
        n = ctypes.c_size_t()
        h.call("ivit_range_workspace_bytes", self.nq, self.rows, self.dim, 0, ctypes.byref(n))
        self.ws = torch.empty(max(n.value, 8), dtype=torch.uint8, device="cuda")
        self.row_ptr = torch.zeros(self.nq + 1, dtype=torch.int64, device="cuda")
        self.common = (P(q), self.nq, P(g), self.rows, self.dim, P(w), P(qw), float(thr), 0, 0, int(triangle), 0, P(self.ws), self.ws.numel())
        self.keep = (q, g, w, qw)
        self.count()
        self.total = int(self.row_ptr[self.nq].item())
        self.idx = torch.empty(max(self.total, 1), dtype=torch.int32, device="cuda")
        self.val = torch.empty(max(self.total, 1), dtype=torch.float32, device="cuda")

    def count(self):
        self.h.call("ivit_range_count", *self.common, P(self.row_ptr))

    def fill(self):
        self.h.call("ivit_range_fill", *self.common, self.total, P(self.idx), P(self.val))


def rows_int8(n, dim, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(-128, 128, (n, dim), generator=g, device="cuda", dtype=torch.int32).to(torch.int8)


def inv_norms(h, x):
    out = torch.empty(x.shape[0], dtype=torch.float32, device="cuda")
    h.call("ivit_gallery_inv_norms", P(x), x.shape[0], x.shape[1], P(out))
    return out


def thresholds(q, g, w, qw):
    """thresholds at which about 0, 1e-4 and 1e-2 of the scores hit, from the scores of 64 queries against 65536 rows"""
    v = (q[:64].float() @ g[:65536].float().T) * w[:65536][None, :]
    if qw is not None:
        v = v * qw[:64, None]
    v = v.flatten()
    return {"0": float(v.max().item()) * 4 + 1.0, "1e-4": float(torch.quantile(v[:1 << 22], 1 - 1e-4).item()),
            "1e-2": float(torch.quantile(v[:1 << 22], 1 - 1e-2).item())}


def check(h, q, g, w, qw, thr, triangle):
    n, m = min(64, q.shape[0]), min(4096, g.shape[0])
    r = Range(h, q[:n].contiguous(), g[:m].contiguous(), w[:m].contiguous(), None if qw is None else qw[:n].contiguous(), thr, triangle)
    r.fill()
    torch.cuda.synchronize()
    ref = range_reference(q[:n].cpu().numpy(), g[:m].cpu().numpy(), w[:m].cpu().numpy(), None if qw is None else qw[:n].cpu().numpy(), thr, 0, 0,
                          triangle)
    assert np.array_equal(r.row_ptr.cpu().numpy(), ref[0]) and np.array_equal(r.idx.cpu().numpy()[:r.total], ref[1])
    assert np.array_equal(r.val.cpu().numpy()[:r.total].view(np.uint32), ref[2].view(np.uint32))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--dim", type=int, nargs="+", default=[384, 768])
    ap.add_argument("--rows", type=int, nargs="+", default=[131072, 1048576])
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--self-join", type=int, default=131072, help="rows of the self-join (0: skip it)")
    ap.add_argument("--window", type=float, default=0.15)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None, help="a JSON file of all results")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/range_bench.py needs a HIP device: a time is a run on the GPU")
    h = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    results = []
    smallest = (min(args.rows), min(args.dim))
    for rows in args.rows:
        for dim in args.dim:
            g, q = rows_int8(rows, dim, rows + dim), rows_int8(args.nq, dim, rows + dim + 1)
            w = inv_norms(h, g)
            n = ctypes.c_size_t()
            h.call("ivit_search_workspace_bytes", args.nq, rows, dim, 1, 0, ctypes.byref(n))
            sws = torch.empty(max(n.value, 8), dtype=torch.uint8, device="cuda")
            sidx = torch.empty(args.nq, 1, dtype=torch.int32, device="cuda")
            sval = torch.empty(args.nq, 1, dtype=torch.float32, device="cuda")
            topk = lambda: h.call("ivit_search_topk", P(q), args.nq, P(g), rows, dim, P(w), 1, 0, 0, P(sws), sws.numel(), P(sidx), P(sval))  # noqa: E731
            for name, thr in thresholds(q, g, w, None).items():
                check(h, q, g, w, None, thr, False)
                r = Range(h, q, g, w, None, thr)
                t = interleaved({"count": r.count, "fill": r.fill, "topk1": topk}, args.window, args.repeat)
                res = {"case": "search", "rows": rows, "dim": dim, "nq": args.nq, "rate": name, "hits_per_score": r.total / (args.nq * rows),
                       "count_ms": round(t["count"][0], 4), "count_ms_range": t["count"][1], "fill_ms": round(t["fill"][0], 4),
                       "fill_ms_range": t["fill"][1], "topk1_ms": round(t["topk1"][0], 4), "topk1_ms_range": t["topk1"][1],
                       "count_over_topk1": round(t["count"][0] / t["topk1"][0], 4)}
                if (rows, dim) == smallest:
                    acc = torch.empty(args.nq, rows, dtype=torch.int32, device="cuda")

                    def matrix():
                        h.call("ivit_linear_i8", P(q), P(g), None, P(acc), args.nq, rows, dim)
                        return torch.nonzero((acc.float() * w[None, :]) >= thr)
                    try:
                        m = interleaved({"matrix": matrix}, args.window, args.repeat)["matrix"]
                        res.update(matrix_ms=round(m[0], 4), matrix_ms_range=m[1])
                    except _lib.IvitError as e:                 # the matrix route refuses the shape: say so, time the rest
                        res.update(matrix_error=str(e))
                    del acc
                results.append(res)
                print(json.dumps(res), flush=True)
                del r
            del g, q, w, sws
            torch.cuda.empty_cache()
    if args.self_join:
        n, dim = args.self_join, args.dim[0]
        x = rows_int8(n, dim, n + dim + 2)
        w = inv_norms(h, x)
        thr = thresholds(x, x, w, w)["1e-4"]
        check(h, x, x, w, w, thr, True)
        full, tri = Range(h, x, x, w, w, thr, False), Range(h, x, x, w, w, thr, True)
        t = interleaved({"count_full": full.count, "count_tri": tri.count, "fill_full": full.fill, "fill_tri": tri.fill}, args.window, args.repeat)
        waves = (n + 31) // 32                           # a wavefront of 32 queries at q0 loads the tiles from q0 // 32 on (its part allowing)
        tiles_full, tiles_tri = waves * waves, waves * (waves + 1) // 2
        res = {"case": "self-join", "rows": n, "dim": dim, "hits_per_score": full.total / (n * n), "pairs": tri.total,
               "tiles_ratio": round(tiles_tri / tiles_full, 4)}
        for name, (ms, rng) in t.items():
            res[name + "_ms"], res[name + "_ms_range"] = round(ms, 4), rng
        res["count_tri_over_full"] = round(t["count_tri"][0] / t["count_full"][0], 4)
        res["fill_tri_over_full"] = round(t["fill_tri"][0] / t["fill_full"][0], 4)
        results.append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
