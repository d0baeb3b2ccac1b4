"""Timing of hidden states on the device (profiles/README.md, "Hidden states"): DeiT-S and Swin-T at batch 256, engine.forward beside
engine.hidden_states tapping the last block / all stages — int16 only (for a ViT the cost of the last block run on all rows instead
of the class-token tail), and with each fp32 layout; and the fp32 launch alone, ivit_hidden_f32 per plane in both layouts, beside a
device-to-device hipMemcpyAsync of a buffer of the plane's fp32 size in the same loop (the copy moves 4 + 4 bytes per element, the
kernel 2 + 4).  The method is tools/topk_bench.py's: the variants alternate inside one loop, HIP-event times, medians with quartiles
and extremes, differences taken round by round.  Prints one JSON line per measurement.
    python tools/hidden_bench.py [--reps 50] [--batch 256]"""
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
from ivit_amd.predict import hidden_reference  # noqa: E402
from topk_bench import interleaved, spread  # noqa: E402

_P = ctypes.c_void_p


def bench_operator(reps, B, planes):
    """`planes`: (name, T, C, t0) — the fp32 launch of one plane in both layouts beside a copy of its fp32 bytes"""
    H = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(0)
    for name, T, C, t0 in planes:
        q = rng.integers(-32768, 32768, size=(B, T, C), dtype=np.int64).astype(np.int16)
        x = torch.from_numpy(q).cuda()
        n32 = B * (T - t0) * C
        out, src = torch.empty(n32, dtype=torch.float32, device="cuda"), torch.zeros(n32, dtype=torch.float32, device="cuda")
        scale = 0.00123
        call = lambda layout: H.call("ivit_hidden_f32", _P(x.data_ptr()), scale, B, T, C, t0, layout, _P(out.data_ptr()))      # noqa: E731
        same = {}
        for lname, layout in (("tokens", _lib.IVIT_HIDDEN_TOKENS), ("grid", _lib.IVIT_HIDDEN_GRID)):
            call(layout)
            torch.cuda.synchronize()
            want = hidden_reference(q[:2], scale, lname, t0)                     # two images: the rest is the same code path
            got = out.cpu().numpy().reshape((B,) + want.shape[1:])[:2]
            same[lname] = bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
        variants = {"tokens": lambda: call(_lib.IVIT_HIDDEN_TOKENS), "grid": lambda: call(_lib.IVIT_HIDDEN_GRID),
                    "copy_d2d_fp32_size": lambda: out.copy_(src, non_blocking=True)}
        t, rounds = interleaved(variants, reps)
        diff = {f"{a}_minus_{b}": spread(np.asarray(rounds[a]) - np.asarray(rounds[b]))
                for a, b in (("tokens", "copy_d2d_fp32_size"), ("grid", "tokens"))}
        print(json.dumps({"what": "ivit_hidden_f32 vs a copy", "plane": name, "shape": {"B": B, "T": T, "C": C, "t0": t0},
                          "fp32_megabytes": round(n32 * 4 / 1e6, 2), "single_call_us": t, "differences_us_per_round": diff,
                          "equal_to_reference": same}), flush=True)


def bench_model(name, golden, B, reps, nslices):
    g = np.load(os.path.join(ROOT, "tests", "golden", golden))
    scales = {k[len("scale/"):]: np.float32(g[k]) for k in g.files if k.startswith("scale/")}
    swin = name in iv.SWIN_CONFIGS
    if swin:
        from ivit_amd.swin_engine import SwinEngine
        cfg = iv.SWIN_CONFIGS[name]
        eng = SwinEngine(cfg, iv.make_swin_weights(cfg, int(g["seed"])), scales)
        sites = tuple(range(cfg.num_layers))
    else:
        from ivit_amd.engine import ViTEngine
        cfg = iv.CONFIGS[name]
        eng = ViTEngine.from_float(cfg, iv.make_vit_weights(cfg, int(g["seed"])), scales)
        sites = (cfg.depth - 1,)
    imgs = torch.from_numpy(iv.make_images_int8(cfg, B, seed=101)).cuda()
    variants = {"forward": lambda: eng.forward(imgs, nslices=nslices),
                "hidden_int16": lambda: eng.hidden_states(imgs, sites, logits=True, nslices=nslices),
                "hidden_tokens": lambda: eng.hidden_states(imgs, sites, layout="tokens", logits=True, nslices=nslices),
                "hidden_grid": lambda: eng.hidden_states(imgs, sites, layout="grid", logits=True, nslices=nslices)}
    fwd = eng.forward(imgs, nslices=nslices, copy=True)
    same = True
    for layout in (None, "tokens", "grid"):
        out = eng.hidden_states(imgs, sites, layout=layout, logits=True, nslices=nslices)
        same = same and bool(torch.equal(out[2], fwd))
    t, rounds = interleaved(variants, reps, warmup=5)
    diff = {f"{a}_minus_{b}": spread(np.asarray(rounds[a]) - np.asarray(rounds[b]))
            for a, b in (("hidden_int16", "forward"), ("hidden_tokens", "hidden_int16"), ("hidden_grid", "hidden_int16"))}
    print(json.dumps({"what": "hidden_states vs forward", "model": name, "batch": B, "nslices": nslices, "sites": list(sites), "rounds": reps,
                      "us": t, "differences_us_per_round": diff, "same_logits": same}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    B = args.batch
    bench_operator(2 * args.reps, B, [("deit_small block", 197, 384, 1), ("swin_tiny stage 0", 3136, 96, 0), ("swin_tiny stage 3", 49, 768, 0)])
    bench_model("deit_small", "deit_small_b4.npz", B, args.reps, 1)
    bench_model("swin_tiny", "swin_tiny_b1.npz", B, args.reps, 2)


if __name__ == "__main__":
    main()
