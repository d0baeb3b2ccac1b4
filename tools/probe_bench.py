"""Timing of ivit_probe_accumulate on the device (profiles/README.md, "Linear probe"): seeded random int8 features of (256 x 384),
(256 x 768) and (65 536 x 384) with 1000 classes.  In one process, alternating inside one loop (the method of tools/topk_bench.py:
HIP-event times, medians with quartiles and extremes):
  (a) the route without this entry: torch `x.double().T @ x.double()` into the Gram matrix, `index_add_` of the rows into the class
      sums and of ones into the counts — exact in float64 up to 2^53, converted to int64 for the comparison;
  (b) ivit_probe_accumulate, and (b) at forced numbers of parts.
Then the share of a DeiT-S batch-256 `features` call that one accumulate of its 256 x 384 features takes (--no-model skips it).
Prints one JSON line per shape and one for the model.
    python tools/probe_bench.py [--reps 30]"""
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
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from topk_bench import interleaved  # noqa: E402

_P = ctypes.c_void_p


def P(t):
    return _P(t.data_ptr())


def bench(H, rows, dim, C, reps, parts_list):
    gen = torch.Generator(device="cuda").manual_seed(rows + dim)
    x = torch.randint(-128, 128, (rows, dim), generator=gen, device="cuda", dtype=torch.int32).to(torch.int8)
    lab = torch.randint(0, C, (rows,), generator=gen, device="cuda", dtype=torch.int64)
    gram, csum, cnt = (torch.zeros(*s, dtype=torch.int64, device="cuda") for s in ((dim, dim), (C, dim), (C,)))
    tg, ts, tc = (torch.zeros(*s, dtype=torch.float64, device="cuda") for s in ((dim, dim), (C, dim), (C,)))
    ones = torch.ones(rows, dtype=torch.float64, device="cuda")

    def ours(parts):
        return lambda: H.call("ivit_probe_accumulate", P(x), P(lab), rows, dim, C, parts, P(gram), P(csum), P(cnt))

    def torch_route():
        xd = x.double()
        tg.add_(xd.T @ xd)
        ts.index_add_(0, lab, xd)
        tc.index_add_(0, lab, ones)

    ours(0)()
    torch_route()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(a, b.to(torch.int64))) for a, b in ((gram, tg), (csum, ts), (cnt, tc)))
    variants = {"torch_double_matmul_index_add": torch_route, "probe_accumulate": ours(0)}
    for p in parts_list:
        variants[f"probe_accumulate_parts_{p}"] = ours(p)
    t, _ = interleaved(variants, reps, warmup=3)
    print(json.dumps({"what": "probe accumulate", "rows": rows, "dim": dim, "classes": C, "rounds": reps, "us": t, "equal_to_torch": same,
                      "torch_over_ours": round(t["torch_double_matmul_index_add"]["median"] / t["probe_accumulate"]["median"], 2)}), flush=True)


def bench_model(reps, C):
    from ivit_amd.engine import ViTEngine
    from ivit_amd.probe import ProbeStats
    g = np.load(os.path.join(ROOT, "tests", "golden", "deit_small_b4.npz"))
    cfg = iv.CONFIGS["deit_small"]
    scales = {k[len("scale/"):]: np.float32(g[k]) for k in g.files if k.startswith("scale/")}
    eng = ViTEngine.from_float(cfg, iv.make_vit_weights(cfg, int(g["seed"])), scales)
    B = 256
    imgs = torch.from_numpy(iv.make_images_int8(cfg, B, seed=101)).cuda()
    lab = torch.randint(0, C, (B,), device="cuda", dtype=torch.int64)
    stats = ProbeStats(eng.num_features, C, eng.device)
    feat8 = eng.features(imgs)[0]
    variants = {"features": lambda: eng.features(imgs), "accumulate": lambda: stats.add(feat8, lab),
                "probe_accumulate": lambda: eng.probe_accumulate(imgs, lab, stats)}
    t, _ = interleaved(variants, reps, warmup=3)
    print(json.dumps({"what": "DeiT-S b256: features, one accumulate of its features, both", "classes": C, "rounds": reps, "us": t,
                      "accumulate_share_of_features": round(t["accumulate"]["median"] / t["features"]["median"], 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--parts", type=int, nargs="*", default=[1, 64], help="forced numbers of parts timed beside the library's choice")
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    assert args.reps >= 20, "at least 20 repetitions of each"
    H = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    for rows, dim in ((256, 384), (256, 768), (65536, 384)):
        bench(H, rows, dim, args.classes, args.reps, args.parts)
    if not args.no_model:
        bench_model(args.reps, args.classes)


if __name__ == "__main__":
    main()
