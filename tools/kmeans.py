"""Exact integer k-means of a frozen model's int8 features over a file of images (include/ivit_cluster.h, ivit_amd/cluster.py).

    python tools/kmeans.py data.npz --model deit_tiny --golden tests/golden/deit_tiny_b1.npz --k 256 --iters 20 --out clusters.npz
    python tools/kmeans.py data.npz --model-file deit_small.ivit --k 1000 --out clusters.npz --seed 3

data.npz and the model are given as to tools/embed.py (the same loading code); `labels` is optional.  The images are embedded once
(`predict.kmeans_fit`: the int8 features of the dataset are kept on the device), the centroids seeded by --init on the host from
--seed, then --iters Lloyd iterations of three launches each.  Writes to --out
  centroids  int8 [K, num_features]     after the last update
  assign     int32 [N]                  every image's nearest centroid (against those centroids)
  dist2      int32 [N]                  its exact squared distance, in units of the features' scale squared
  inertia    int64 [iters]              the inertia of every iteration's assignment (need not fall: the means are rounded to int8)
  scale      float32                    the features' scale
  purity, nmi  float64                  with labels in data.npz: the clustering against them
and prints one JSON line.  One device."""
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
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--init", choices=("kmeans++", "sample"), default="kmeans++")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True, help="the .npz to write")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/kmeans.py needs a HIP device; the product path has no CPU fallback")
    from ivit_amd import cluster
    from ivit_amd.predict import kmeans_fit
    device = "cuda:0"
    cfg, eng, s_in = build_engine(args, device)
    d = np.load(args.data)
    n = len(d["offsets"]) if "pixels" in d.files else len(d["images"])
    labels = d["labels"].astype(np.int64).reshape(-1) if "labels" in d.files else np.zeros(0, np.int64)
    mine, transform = load_share(d, labels if len(labels) else np.zeros(n, np.int64), cfg, s_in, args, device, 0, n)
    batches = (mine[a:a + args.batch] for a in range(0, n, args.batch))
    km, feat8, inertia = kmeans_fit(eng, batches, args.k, iters=args.iters, init=args.init, generator=np.random.default_rng(args.seed),
                                    transform=transform)
    assign, dist2 = km.assign(feat8)
    out = dict(centroids=km.numpy()[0], assign=assign.cpu().numpy(), dist2=dist2.cpu().numpy(), inertia=inertia,
               scale=np.float32(eng.feature_scale_host()))
    line = {"n": int(n), "k": int(args.k), "iters": int(len(inertia)), "inertia": int(inertia[-1]) if len(inertia) else None,
            "moved_last": int(getattr(km, "last_moved", 0)), "model": args.model, "out": args.out}
    if len(labels):
        C = int(labels.max()) + 1
        table = cluster.contingency(assign, torch.from_numpy(labels).to(assign.device), args.k, C)
        out["purity"], out["nmi"] = np.float64(cluster.purity(table)), np.float64(cluster.nmi(table))
        line.update(purity=float(out["purity"]), nmi=float(out["nmi"]))
    np.savez(args.out, **out)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
