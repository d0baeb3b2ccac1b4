"""Timing of the class-token attention tap on the device (profiles/README.md, "Attention maps"): DeiT-S batch 256,
engine.attention(blocks=-1, logits=True) and engine.attention(blocks=-1, logits=False) beside engine.forward on the same images,
and the tap launch alone (ivit_attention_cls_probs on 256 x 6 heads, T = 197, dh = 64) and the map launch alone.  The method is
tools/topk_bench.py's: the variants alternate inside one loop, HIP-event times, medians with quartiles and extremes, differences
taken round by round.  Prints one JSON line per measurement.   python tools/attention_bench.py [--reps 100]"""
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
from ivit_amd.predict import attention_map_reference, attention_reference  # noqa: E402
from topk_bench import interleaved, spread  # noqa: E402

_P = ctypes.c_void_p


def bench_operator(reps):
    H = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    B, nh, T, dh = 256, 6, 197, 64
    rng = np.random.default_rng(0)
    q = rng.integers(-128, 128, size=(B * nh, T, dh), dtype=np.int64).astype(np.int8)
    k = rng.integers(-128, 128, size=(B * nh, T, dh), dtype=np.int64).astype(np.int8)
    dq, dk = torch.from_numpy(q).cuda(), torch.from_numpy(k).cuda()
    p = torch.empty(B * nh * T, dtype=torch.int16, device="cuda")
    out = torch.empty(B * nh * (T - 1), dtype=torch.float32, device="cuda")
    dy, s = _lib.Dyadic(float(round(2.0 ** 31 / 1.37)), 2.0 ** -41), 0.0725
    tap = lambda: H.call("ivit_attention_cls_probs", _P(dq.data_ptr()), _P(dk.data_ptr()), dy, s, _P(p.data_ptr()), B, nh, T, dh)      # noqa: E731
    fmap = lambda mode: H.call("ivit_attention_map_f32", _P(p.data_ptr()), B, nh, T, mode, _P(out.data_ptr()))                         # noqa: E731
    tap()
    torch.cuda.synchronize()
    got = p.cpu().numpy().view(np.uint16).reshape(B * nh, T)
    same = bool(np.array_equal(got, attention_reference(q, k, (dy.m, dy.r), s)))
    for mode, heads in ((0, True), (1, False)):
        fmap(mode)
        torch.cuda.synchronize()
        want = attention_map_reference(got.reshape(B, nh, T), heads=heads)
        same = same and bool(np.array_equal(out.cpu().numpy()[:want.size].view(np.uint32), want.reshape(-1).view(np.uint32)))
    variants = {"cls_probs": tap, "map_heads": lambda: fmap(0), "map_mean": lambda: fmap(1)}
    print(json.dumps({"what": "attention tap and map launches", "shape": {"B": B, "H": nh, "T": T, "dh": dh},
                      "single_call_us": interleaved(variants, reps)[0],
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
                "attention_with_logits": lambda: eng.attention(imgs, blocks=-1, logits=True),
                "attention_headless": lambda: eng.attention(imgs, blocks=-1)}
    fwd = eng.forward(imgs, copy=True)
    a16, _, logits = eng.attention(imgs, blocks=-1, logits=True, copy=True)
    same = bool(torch.equal(logits, fwd)) and bool(torch.equal(eng.attention(imgs, blocks=-1)[0].view(torch.int16), a16.view(torch.int16)))
    t, rounds = interleaved(variants, reps, warmup=5)
    diff = {k: spread(np.asarray(rounds[k]) - np.asarray(rounds["forward"])) for k in ("attention_with_logits", "attention_headless")}
    print(json.dumps({"what": "attention vs forward", "model": name, "batch": B, "rounds": reps, "us": t,
                      "minus_forward_us_per_round": diff,
                      "with_logits_minus_forward_pct_of_forward_median":
                          round(100.0 * diff["attention_with_logits"]["median"] / t["forward"]["median"], 3),
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
