"""Timing of features on the device (profiles/README.md, "Features"): DeiT-S batch 256, engine.features(logits=False) — the
backbone into the caller's rows and the fp32 launch, no head GEMM — beside engine.forward and engine.features(logits=True) on the
same images, and the fp32 launch alone in both modes on 256 x 384 rows.  The method is tools/topk_bench.py's: the variants
alternate inside one loop, HIP-event times, medians with quartiles and extremes, differences taken round by round.  Prints one
JSON line per measurement.   python tools/features_bench.py [--reps 100]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from ivit_amd.predict import features_reference  # noqa: E402
from topk_bench import interleaved, spread  # noqa: E402

_P = ctypes.c_void_p


def bench_operator(reps):
    H = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    q = np.random.default_rng(0).integers(-128, 128, size=(256, 384), dtype=np.int64).astype(np.int8)
    feat8 = torch.from_numpy(q).cuda()
    out = torch.empty(256, 384, dtype=torch.float32, device="cuda")
    args = lambda mode: (_P(feat8.data_ptr()), 256, 384, 0.03, mode, _P(out.data_ptr()))      # noqa: E731
    variants = {"dequant": lambda: H.call("ivit_features_f32", *args(0)), "unit": lambda: H.call("ivit_features_f32", *args(1))}
    same = True
    for mode in (0, 1):
        H.call("ivit_features_f32", *args(mode))
        torch.cuda.synchronize()
        same = same and bool(np.array_equal(out.cpu().numpy().view(np.uint32), features_reference(q, 0.03, mode).view(np.uint32)))
    print(json.dumps({"what": "features_f32 launch", "shape": [256, 384], "single_call_us": interleaved(variants, reps)[0],
                      "train_of_20_us_per_call": interleaved(variants, max(20, reps // 4), train=20)[0],
                      "equal_to_reference": same}), flush=True)


def bench_model(name, golden, B, reps):
    g = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", golden))
    cfg = iv.CONFIGS[name]
    scales = {k[len("scale/"):]: np.float32(g[k]) for k in g.files if k.startswith("scale/")}
    from ivit_amd.engine import ViTEngine
    eng = ViTEngine.from_float(cfg, iv.make_vit_weights(cfg, int(g["seed"])), scales)
    imgs = torch.from_numpy(iv.make_images_int8(cfg, B, seed=101)).cuda()
    variants = {"forward": lambda: eng.forward(imgs),
                "features": lambda: eng.features(imgs),
                "features_with_logits": lambda: eng.features(imgs, logits=True)}
    fwd = eng.forward(imgs, copy=True)
    f8, _, logits = eng.features(imgs, logits=True, copy=True)
    same = bool(torch.equal(logits, fwd)) and bool(torch.equal(eng.features(imgs)[0], f8))
    t, rounds = interleaved(variants, reps, warmup=5)
    diff = {k: spread(np.asarray(rounds[k]) - np.asarray(rounds["forward"])) for k in ("features", "features_with_logits")}
    print(json.dumps({"what": "features vs forward", "model": name, "batch": B, "rounds": reps, "us": t,
                      "minus_forward_us_per_round": diff,
                      "features_minus_forward_pct_of_forward_median": round(100.0 * diff["features"]["median"] / t["forward"]["median"], 3),
                      "same_integers": same}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    bench_operator(2 * args.reps)
    bench_model("deit_small", "deit_small_b4.npz", 256, args.reps)


if __name__ == "__main__":
    main()
