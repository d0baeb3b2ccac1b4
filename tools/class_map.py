"""Class-activation maps of a frozen Swin over a file of images: the head's weight row of a class against every final-stage token,
in exact integers, on the native engine (SwinEngine.class_map, include/ivit_classmap.h).

    python tools/class_map.py data.npz --model swin_tiny --golden tests/golden/swin_tiny_b1.npz --out maps.npz
    python tools/class_map.py data.npz --model swin_tiny --state-dict checkpoint.pth.tar --labels --out maps.npz

data.npz and the model are given as to tools/attention_map.py, tools/embed.py and tools/evaluate.py (the same loading code: int8
model inputs, uint8 [N, H, W, 3] images or a packed ragged file; --golden or --state-dict).  Without --labels the maps are those of
the --topk best classes of every image; with --labels those of the file's `labels`, one class per image (a label outside the classes
gives a map of zeros / NaN).  Writes to --out
  idx          int32 [N, k]            the classes of the maps: the predictions, or the labels
  val          float32 [N, k]          the predictions' dequantised head outputs (empty [N, 0] with --labels)
  tok8         int8 [N, L, C]          the final-stage tokens behind norm -> qact2, L = gh * gw in row-major grid order
  token_scale  float32                 their scale (qact2)
  cam32        int32 [N, k, L]         head_w[class] . tok8[n, t]: exact
  maps         float32 [N, k, gh, gw]  cam32 * fl32(token_scale * fc_scaling_factor[class]) on the token grid
  labels       int64 [N]               copied from data.npz (empty if it has none)
Prints one JSON line {"n", "k", "given", "grid", "model", "out"}.  One device.  Swin only: a ViT's patch rows have no scale."""
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
    ap.add_argument("--topk", type=int, default=5, help="maps of the K best classes of every image (default 5)")
    ap.add_argument("--labels", action="store_true", help="maps of the file's labels instead, one class per image")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/class_map.py needs a HIP device; the product path has no CPU fallback")
    device = "cuda:0"
    cfg, eng, s_in = build_engine(args, device)
    if not hasattr(eng, "class_map"):
        raise SystemExit(f"--model {args.model}: class-activation maps are a Swin feature (a ViT's patch rows have no scale)")
    d = np.load(args.data)
    n = len(d["offsets"]) if "pixels" in d.files else len(d["images"])
    labels = d["labels"].astype(np.int64).reshape(-1) if "labels" in d.files else np.zeros(0, np.int64)
    if args.labels and len(labels) != n:
        raise SystemExit("--labels: data.npz has no `labels` for every image")
    mine, transform = load_share(d, labels if len(labels) else np.zeros(n, np.int64), cfg, s_in, args, device, 0, n)
    k = 1 if args.labels else args.topk
    g = cfg.grid >> (cfg.num_layers - 1)
    parts = {name: [] for name in ("idx", "val", "tok8", "cam32", "maps")}
    for a in range(0, n, args.batch):
        images = mine[a:a + args.batch]
        classes = torch.from_numpy(labels[a:a + args.batch].astype(np.int32).reshape(-1, 1)).to(device) if args.labels else None
        out = eng.class_map(transform(images) if transform is not None else images, k=k, classes=classes)
        for name, t in zip(parts, out):
            parts[name].append(np.zeros((len(images), 0), np.float32) if t is None else t.cpu().numpy())
    empty = {"idx": ((0, k), np.int32), "val": ((0, 0 if args.labels else k), np.float32), "tok8": ((0, g * g, eng.num_features), np.int8),
             "cam32": ((0, k, g * g), np.int32), "maps": ((0, k, g, g), np.float32)}
    arrays = {name: np.concatenate(v) if v else np.zeros(*empty[name]) for name, v in parts.items()}
    np.savez(args.out, token_scale=np.float32(eng.token_scale_host()), labels=labels, **arrays)
    print(json.dumps({"n": int(n), "k": int(k), "given": bool(args.labels), "grid": [g, g], "model": args.model, "out": args.out}))


if __name__ == "__main__":
    main()
