"""Timing of the prediction path on the device (profiles/README.md, "Predictions"):
  * ivit_logits_topk at (256, 1000, 5) and (1, 1000, 5) beside torch.topk(logits.float() * scale, 5) on the same buffers;
  * engine.predict beside engine.forward, and beside forward followed by the torch route, for DeiT-S b256 and DeiT-T b1.
Every figure is a median of HIP-event times, printed with its quartiles and extremes; the variants of one comparison alternate
inside one loop, so they see the same box at the same moment.  A single small launch is near the events' own resolution, so each is also timed as a train of 20 launches
between one pair of events.  Prints one JSON line per comparison.   python tools/topk_bench.py [--reps 200]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402

_P = ctypes.c_void_p


def timed(fn, train=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(train):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / train          # microseconds per call


def interleaved(variants, reps, train=1, warmup=10):
    """({name: spread in us}, {name: every round's time}) — one call (or train) of every variant per round, in turn"""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            t[k].append(timed(fn, train))
    return {k: spread(v) for k, v in t.items()}, t


def spread(v):
    """median, quartiles and extremes of a list of times"""
    q = np.percentile(np.asarray(v, dtype=np.float64), [50, 25, 75, 0, 100])
    return dict(zip(("median", "q25", "q75", "min", "max"), (round(float(x), 2) for x in q)))


def bench_operator(reps):
    H = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(0)
    for B in (256, 1):
        logits = torch.from_numpy(rng.integers(-2 ** 20, 2 ** 20, size=(B, 1000), dtype=np.int64).astype(np.int32)).cuda()
        scale = torch.from_numpy(rng.uniform(1e-4, 1e-3, size=1000).astype(np.float32)).cuda()
        idx = torch.empty(B, 5, dtype=torch.int32, device="cuda")
        val = torch.empty(B, 5, dtype=torch.float32, device="cuda")
        args = (_P(logits.data_ptr()), _P(scale.data_ptr()), B, 1000, 5, _P(idx.data_ptr()), _P(val.data_ptr()))
        variants = {"ivit_logits_topk": lambda: H.call("ivit_logits_topk", *args),
                    "torch_mul_topk": lambda: torch.topk(logits.float() * scale, 5)}
        tv, ti = torch.topk(logits.float() * scale, 5)
        H.call("ivit_logits_topk", *args)
        torch.cuda.synchronize()
        same = bool(torch.equal(val, tv)) and bool(torch.equal(idx.long(), ti))      # untied random rows: torch's order is ours
        print(json.dumps({"what": "top-k launch", "shape": [B, 1000, 5], "single_call_us": interleaved(variants, reps)[0],
                          "train_of_20_us_per_call": interleaved(variants, max(20, reps // 4), train=20)[0], "equal_to_torch": same}), flush=True)


def bench_model(name, golden, B, reps):
    g = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", golden))
    cfg = iv.CONFIGS[name]
    scales = {k[len("scale/"):]: np.float32(g[k]) for k in g.files if k.startswith("scale/")}
    from ivit_amd.engine import ViTEngine
    eng = ViTEngine.from_float(cfg, iv.make_vit_weights(cfg, int(g["seed"])), scales)
    imgs = torch.from_numpy(iv.make_images_int8(cfg, B, seed=101)).cuda()
    scale = torch.from_numpy(eng.head_scale_host()).cuda()
    variants = {"forward": lambda: eng.forward(imgs),
                "predict": lambda: eng.predict(imgs, k=5),
                "forward_then_torch_topk": lambda: torch.topk(eng.forward(imgs).float() * scale, 5)}
    idx, val = eng.predict(imgs, k=5, copy=True)
    tv, ti = torch.topk(eng.forward(imgs).float() * scale, 5)
    same_val = bool(torch.equal(val, tv))
    t, rounds = interleaved(variants, reps, warmup=5)
    # the difference is taken round by round (predict and forward of one round run back to back), then summarised
    diff = spread(np.asarray(rounds["predict"]) - np.asarray(rounds["forward"]))
    print(json.dumps({"what": "predict vs forward", "model": name, "batch": B, "rounds": reps, "us": t,
                      "predict_minus_forward_us_per_round": diff,
                      "predict_minus_forward_pct_of_forward_median": round(100.0 * diff["median"] / t["forward"]["median"], 3),
                      "values_equal_torch": same_val, "indices_equal_torch": bool(torch.equal(idx.long(), ti))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    bench_operator(args.reps)
    bench_model("deit_small", "deit_small_b4.npz", 256, max(30, args.reps // 2))
    bench_model("deit_tiny", "deit_tiny_b1.npz", 1, args.reps)


if __name__ == "__main__":
    main()
