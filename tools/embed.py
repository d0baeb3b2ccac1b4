"""Embeddings of a frozen model over a file of images: the reference's forward_features (vit_quant.py:254-276,
swin_quant.py:540-556) on the native engine, without the head.

    python tools/embed.py data.npz --model deit_tiny --golden tests/golden/deit_tiny_b1.npz --out feats.npz
    python tools/embed.py data.npz --model deit_small --state-dict checkpoint.pth.tar --batch 128 --out feats.npz --unit

data.npz and the model are given as to tools/evaluate.py (the same loading code: int8 model inputs, uint8 [N, H, W, 3] images or a
packed ragged file; --golden or --state-dict); `labels` is optional here.  Writes to --out
  feat8     int8 [N, num_features]      the integers the head reads (class-token row after norm -> qact2 / pooled row after qact3)
  scale     float32                     their scale: feat8 * scale is what forward_features returns in the reference
  features  float32 [N, num_features]   that product, every bit — or with --unit the rows at unit Euclidean length
  labels    int64 [N]                   copied from data.npz (empty if it has none)
and prints one JSON line {"n", "num_features", "scale", "unit", "model", "out"}.  One device, no head GEMM."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from evaluate import add_input_arguments, build_engine, load_share  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    add_input_arguments(ap)
    ap.add_argument("--out", required=True, help="the .npz to write")
    ap.add_argument("--unit", action="store_true", help="`features` at unit Euclidean length instead of feat8 * scale")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/embed.py needs a HIP device; the product path has no CPU fallback")
    device = "cuda:0"
    cfg, eng, s_in = build_engine(args, device)
    d = np.load(args.data)
    n = len(d["offsets"]) if "pixels" in d.files else len(d["images"])
    labels = d["labels"].astype(np.int64).reshape(-1) if "labels" in d.files else np.zeros(0, np.int64)
    mine, transform = load_share(d, labels if len(labels) else np.zeros(n, np.int64), cfg, s_in, args, device, 0, n)
    feat8, feat32 = [], []
    for a in range(0, n, args.batch):                       # embed()'s loop, keeping the integers too
        images = mine[a:a + args.batch]
        f8, f32 = eng.features(transform(images) if transform is not None else images, normalize=args.unit, copy=True)
        feat8.append(f8)
        feat32.append(f32)
    F = eng.num_features
    feat8 = torch.cat(feat8).cpu().numpy() if feat8 else np.zeros((0, F), np.int8)
    feat32 = torch.cat(feat32).cpu().numpy() if feat32 else np.zeros((0, F), np.float32)
    scale = np.float32(eng.feature_scale_host())
    np.savez(args.out, feat8=feat8, scale=scale, features=feat32, labels=labels)
    print(json.dumps({"n": int(n), "num_features": int(F), "scale": float(scale), "unit": bool(args.unit), "model": args.model,
                      "out": args.out}))


if __name__ == "__main__":
    main()
