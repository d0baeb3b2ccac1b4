"""Times the radix select of include/ivit_kth.h beside what bounds it and what it replaces, on the same box, INTERLEAVED.

    python tools/kth_bench.py [--rows 100000] [--nq 256] [--gallery 1048576] [--dim 384] [--k 64 1000] [--out kth_bench.json]

Self-join (`--rows` clustered rows, cosine) and cross form (`--nq` queries against `--gallery` rows), per k:
  kth_ms                 ivit_kth_similarity, the library's choice of parts (`parts`, `workspace_bytes`: 0 is the one-launch form)
  range4_ms              FOUR ivit_range_count on the same arrays at a threshold nothing reaches: the same number of streams of the
                         other side with no histogram — the floor this design can approach; kth_over_range4 is the ratio
  core_ms                (self-join, k <= 64) ivit_core_similarity at min_pts = k
  torch_ms               (cross form) the fp32 torch route: matmul in chunks of `--chunk` gallery rows into [nq, gallery], the weights,
                         torch.kthvalue
Medians of `--repeat` rounds, one window of each in turn, with [fastest, slowest].  The device results are compared with
`predict.kth_reference` on the first rows before anything is timed.  Prints one JSON line; needs a HIP device."""
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
from ivit_amd import _lib  # noqa: E402
from ivit_amd.predict import kth_reference  # noqa: E402
from density_bench import clustered_rows  # noqa: E402
from range_bench import P, interleaved, inv_norms  # noqa: E402


class Kth:
    """the buffers and the call of one (queries, rows, k)"""

    def __init__(self, h, q, x, w, qw, k, self_join):
        self.h, (self.nq, dim), rows = h, q.shape, x.shape[0]
        n = ctypes.c_size_t()
        h.call("ivit_kth_workspace_bytes", self.nq, rows, dim, 0, int(self_join), ctypes.byref(n))
        self.bytes = n.value
        self.ws = torch.empty(max(n.value, 16), dtype=torch.uint8, device="cuda")
        self.kth, self.above = torch.empty(self.nq, dtype=torch.float32, device="cuda"), torch.empty(self.nq, dtype=torch.int64, device="cuda")
        self.args = (P(q), self.nq, P(x), rows, dim, P(w), P(qw), int(k), int(self_join), 0, P(self.ws), n.value, P(self.kth), P(self.above))

    def __call__(self):
        self.h.call("ivit_kth_similarity", *self.args)


def range4(h, q, x, w, qw):
    """four ivit_range_count over the same arrays, nothing hit"""
    n = ctypes.c_size_t()
    h.call("ivit_range_workspace_bytes", q.shape[0], x.shape[0], x.shape[1], 0, ctypes.byref(n))
    ws, row_ptr = torch.empty(max(n.value, 8), dtype=torch.uint8, device="cuda"), torch.empty(q.shape[0] + 1, dtype=torch.int64, device="cuda")
    args = (P(q), q.shape[0], P(x), x.shape[0], x.shape[1], P(w), P(qw), 3.0e38, 0, 0, 0, 0, P(ws), ws.numel(), P(row_ptr))

    def run(_keep=(ws, row_ptr)):
        for _ in range(4):
            h.call("ivit_range_count", *args)
    return run


def check(h, q, x, w, qw, k, self_join):
    n = min(2048, x.shape[0])
    m = n if self_join else min(64, q.shape[0])
    k = min(k, n)
    xs, ws_ = x[:n].contiguous(), w[:n].contiguous()
    qs, qws = (xs, None) if self_join else (q[:m].contiguous(), qw[:m].contiguous())
    run = Kth(h, qs, xs, ws_, qws, k, self_join)
    run()
    torch.cuda.synchronize()
    kth, above = kth_reference(qs.cpu().numpy(), xs.cpu().numpy(), ws_.cpu().numpy(), None if qws is None else qws.cpu().numpy(), k, self_join)
    assert np.array_equal(run.kth.cpu().numpy().view(np.uint32), kth.view(np.uint32)) and np.array_equal(run.above.cpu().numpy(), above), "the device differs from kth_reference"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--gallery", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--centres", type=int, default=300)
    ap.add_argument("--k", type=int, nargs="+", default=[64, 1000])
    ap.add_argument("--chunk", type=int, default=1 << 17)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/kth_bench.py needs a HIP device: a time is a run on the GPU")
    h = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    dim = args.dim
    res = {"dim": dim, "library": _lib.SO_PATH}

    def report(t, run):
        r = {name + "_ms": round(t[name][0], 4) for name in t}
        r.update({name + "_ms_range": t[name][1] for name in t})
        r.update(kth_over_range4=round(t["kth"][0] / t["range4"][0], 4), workspace_bytes=run.bytes)
        return r

    x = clustered_rows(args.rows, dim, args.centres, args.rows + dim)
    w = inv_norms(h, x)
    for k in args.k:
        check(h, x, x, w, None, k, True)
        run = Kth(h, x, x, w, None, k, True)
        fns = {"kth": run, "range4": range4(h, x, x, w, w)}
        if k <= 64:
            n = ctypes.c_size_t()
            h.call("ivit_core_workspace_bytes", args.rows, dim, k, 0, ctypes.byref(n))
            cws, core = torch.empty(n.value, dtype=torch.uint8, device="cuda"), torch.empty(args.rows, dtype=torch.float32, device="cuda")
            fns["core"] = lambda: h.call("ivit_core_similarity", P(x), args.rows, dim, P(w), k, 0, P(cws), n.value, P(core))      # noqa: E731
        res["self_%dx%d_k%d" % (args.rows, dim, k)] = report(interleaved(fns, args.window, args.repeat), run)
    del x, w

    g, q = clustered_rows(args.gallery, dim, args.centres, args.gallery + dim), clustered_rows(args.nq, dim, args.centres, args.nq + dim + 1)
    w, qw = inv_norms(h, g), inv_norms(h, q)
    scores, qf = torch.empty(args.nq, args.gallery, dtype=torch.float32, device="cuda"), q.float()

    def torch_route(k):
        for c0 in range(0, args.gallery, args.chunk):
            torch.matmul(qf, g[c0:c0 + args.chunk].float().T, out=scores[:, c0:c0 + args.chunk])
        scores.mul_(w[None, :]).mul_(qw[:, None])
        return torch.kthvalue(scores, args.gallery - k + 1, dim=1)[0]
    for k in args.k:
        check(h, q, g, w, qw, k, False)
        run = Kth(h, q, g, w, qw, k, False)
        t = interleaved({"kth": run, "range4": range4(h, q, g, w, qw), "torch": lambda: torch_route(k)}, args.window, args.repeat)
        res["cross_%dx%dx%d_k%d" % (args.nq, args.gallery, dim, k)] = report(t, run)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "result": res}, f, indent=1)


if __name__ == "__main__":
    main()
