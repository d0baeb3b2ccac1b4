"""Density clustering (DBSCAN) of a frozen model's int8 features over a file of images (include/ivit_density.h, ivit_amd/cluster.py).

    python tools/dbscan.py data.npz --model deit_tiny --golden tests/golden/deit_tiny_b1.npz --threshold 0.8 --min-pts 5 --out clusters.npz
    python tools/dbscan.py data.npz --model-file deit_small.ivit --threshold 0.8 --min-pts 5 --out clusters.npz

data.npz and the model are given as to tools/kmeans.py (the same loading code); `labels` is optional.  The images are embedded once
(`predict.dbscan_fit`: the int8 features of the dataset are kept on the device), then clustered on the cosine of their features: a
row with at least --min-pts rows at a cosine >= --threshold (itself among them) is a core row, core rows within the threshold of each
other share a cluster, other rows join the cluster of a core row within reach or are noise.  Writes to --out
  label      int32 [N]      the smallest row of the image's cluster, -1 for noise
  cluster    int32 [N]      the clusters numbered 0 .. n_clusters - 1 in ascending order of label, -1 for noise
  core       bool [N]
  degree     int32 [N]      rows within the threshold, the image itself included
  purity, nmi  float64      with labels in data.npz: the clustering against them, over the rows that are not noise
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
    ap.add_argument("--threshold", type=float, default=0.8, help="the cosine from which two images are neighbours")
    ap.add_argument("--min-pts", type=int, default=5, help="neighbours (the image itself included) that make a core row")
    ap.add_argument("--out", required=True, help="the .npz to write")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/dbscan.py needs a HIP device; the product path has no CPU fallback")
    from ivit_amd import cluster
    from ivit_amd.predict import dbscan_fit
    device = "cuda:0"
    cfg, eng, s_in = build_engine(args, device)
    d = np.load(args.data)
    n = len(d["offsets"]) if "pixels" in d.files else len(d["images"])
    labels = d["labels"].astype(np.int64).reshape(-1) if "labels" in d.files else np.zeros(0, np.int64)
    mine, transform = load_share(d, labels if len(labels) else np.zeros(n, np.int64), cfg, s_in, args, device, 0, n)
    batches = (mine[a:a + args.batch] for a in range(0, n, args.batch))
    label, core, degree, _ = dbscan_fit(eng, batches, args.threshold, args.min_pts, transform=transform)
    compact, count = cluster.compact_labels(label)
    noise = int((label < 0).sum())
    out = dict(label=label.cpu().numpy(), cluster=compact.cpu().numpy(), core=core.cpu().numpy(), degree=degree.cpu().numpy())
    line = {"n": int(n), "threshold": args.threshold, "min_pts": args.min_pts, "clusters": count, "noise_share": noise / max(n, 1),
            "core": int(core.sum()), "model": args.model, "out": args.out}
    if len(labels) and count:
        C = int(labels.max()) + 1
        table = cluster.contingency(compact, torch.from_numpy(labels).to(compact.device), count, C)      # a noise row is out of range: left out
        out["purity"], out["nmi"] = np.float64(cluster.purity(table)), np.float64(cluster.nmi(table))
        line.update(purity=float(out["purity"]), nmi=float(out["nmi"]))
    np.savez(args.out, **out)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
