"""Timing of gallery search on the device (profiles/README.md, "Gallery search"): nq = 256 queries of width 384, k = 16, against
seeded random int8 galleries of 131 072 and 1 048 576 rows (50 MB and 403 MB), cosine weights.  In one process, alternating inside
one loop (the method of tools/topk_bench.py: HIP-event times, medians with quartiles and extremes):
  (a) ivit_linear_i8 + ivit_logits_topk — the library without this feature: the [nq, rows] int32 score matrix is written and read
      back (1.07 GB at the larger size; skipped there with --no-large-baseline or when the allocation fails);
  (b) ivit_search_topk.
Also the fused kernel's bound: operations (2 nq rows dim) over the int8 MFMA peak and gallery bytes over the HBM peak, each over the
measured time, and which of the two binds; and (b) at forced numbers of parts.  Prints one JSON line per size.
    python tools/search_bench.py [--reps 30] [--rows 131072 1048576]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ivit_amd import _lib  # noqa: E402
from topk_bench import interleaved, spread  # noqa: E402

_P = ctypes.c_void_p
INT8_PEAK_OPS = 5.0e15       # dense int8 MFMA, operations per second (MI355X data sheet)
HBM_PEAK_BYTES = 8.0e12      # bytes per second


def P(t):
    return _P(t.data_ptr())


def bench(H, rows, nq, dim, k, reps, baseline, parts_list):
    gen = torch.Generator(device="cuda").manual_seed(rows)
    g = torch.randint(-128, 128, (rows, dim), generator=gen, device="cuda", dtype=torch.int32).to(torch.int8)
    q = torch.randint(-128, 128, (nq, dim), generator=gen, device="cuda", dtype=torch.int32).to(torch.int8)
    w = torch.empty(rows, dtype=torch.float32, device="cuda")
    H.call("ivit_gallery_inv_norms", P(g), rows, dim, P(w))
    idx, val = (torch.empty(nq, k, dtype=dt, device="cuda") for dt in (torch.int32, torch.float32))
    n = ctypes.c_size_t()

    def fused(parts):
        H.call("ivit_search_workspace_bytes", nq, rows, dim, k, parts, ctypes.byref(n))
        ws = torch.empty(max(n.value, 8), dtype=torch.uint8, device="cuda")
        return (lambda: H.call("ivit_search_topk", P(q), nq, P(g), rows, dim, P(w), k, 0, parts, P(ws), ws.numel(), P(idx), P(val))), n.value // (8 * nq * k)

    call, auto_parts = fused(0)
    variants = {"search_topk": call}
    for p in parts_list:
        variants[f"search_topk_parts_{p}"] = fused(p)[0]
    call()
    torch.cuda.synchronize()
    fi, fv = idx.clone(), val.clone()
    same = None
    if baseline:
        try:
            acc = torch.empty(nq, rows, dtype=torch.int32, device="cuda")
        except RuntimeError:
            acc = None
        if acc is not None:
            bi, bv = (torch.empty(nq, k, dtype=dt, device="cuda") for dt in (torch.int32, torch.float32))

            def base():
                H.call("ivit_linear_i8", P(q), P(g), None, P(acc), nq, rows, dim)
                H.call("ivit_logits_topk", P(acc), P(w), nq, rows, k, P(bi), P(bv))
            base()
            torch.cuda.synchronize()
            same = bool(torch.equal(bi, fi)) and bool(torch.equal(bv.view(torch.int32), fv.view(torch.int32)))
            variants = {"linear_i8_then_logits_topk": base, **variants}
    t, rounds = interleaved(variants, reps, warmup=3)
    us = t["search_topk"]["median"]
    ops, nbytes = 2.0 * nq * rows * dim, float(rows) * dim
    out = {"what": "gallery search", "nq": nq, "rows": rows, "dim": dim, "k": k, "gallery_megabytes": round(nbytes / 1e6, 1), "rounds": reps,
           "parts_chosen": int(auto_parts), "us": t, "equal_to_baseline": same,
           "bound": {"mfma_us_at_peak": round(ops / INT8_PEAK_OPS * 1e6, 1), "hbm_us_at_peak": round(nbytes / HBM_PEAK_BYTES * 1e6, 1),
                     "binds": "mfma" if ops / INT8_PEAK_OPS > nbytes / HBM_PEAK_BYTES else "hbm",
                     "fraction_of_int8_peak": round(ops / INT8_PEAK_OPS * 1e6 / us, 4),
                     "fraction_of_hbm_peak": round(nbytes / HBM_PEAK_BYTES * 1e6 / us, 4)}}
    if "linear_i8_then_logits_topk" in rounds:
        out["baseline_minus_fused_us_per_round"] = spread(np.asarray(rounds["linear_i8_then_logits_topk"]) - np.asarray(rounds["search_topk"]))
        out["baseline_over_fused"] = round(t["linear_i8_then_logits_topk"]["median"] / us, 2)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rows", type=int, nargs="*", default=[131072, 1048576])
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--parts", type=int, nargs="*", default=[64, 128, 512], help="forced numbers of parts timed beside the library's choice")
    ap.add_argument("--no-large-baseline", action="store_true", help="no score matrix above 500 MB")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    assert args.reps >= 20, "at least 20 repetitions of each"
    H = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    for rows in args.rows:
        baseline = not (args.no_large_baseline and 4.0 * args.nq * rows > 5e8)
        bench(H, rows, args.nq, args.dim, args.k, args.reps, baseline, args.parts)


if __name__ == "__main__":
    main()
