"""HDBSCAN of a frozen model's int8 features over a file of images (include/ivit_hdbscan.h, ivit_amd/cluster.py): no K, no threshold.

    python tools/hdbscan.py data.npz --model deit_tiny --golden tests/golden/deit_tiny_b1.npz --min-cluster-size 5 --out clusters.npz
    python tools/hdbscan.py data.npz --model-file deit_small.ivit --min-cluster-size 5 --min-pts 10 --out clusters.npz

data.npz and the model are given as to tools/dbscan.py (the same loading code); `labels` is optional.  The images are embedded once
(`predict.hdbscan_fit`: the int8 features of the dataset are kept on the device), then clustered on the cosine of their features: every
image's core similarity (its --min-pts-th largest cosine, itself counted) and the spanning forest of the mutual-reachability values on
the device, the condensed tree and the selection of the most stable clusters on the host.  Writes to --out
  label      int32 [N]      the smallest row of the image's cluster, -1 for noise
  cluster    int32 [N]      the clusters numbered 0 .. n_clusters - 1 in ascending order of label, -1 for noise
  core       float32 [N]    the core similarities
  edge_u, edge_v, edge_val  the forest, in the edge order
  stability  float64 [clusters of the condensed tree], with `birth` and `name` (the smallest row) beside it
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
    ap.add_argument("--min-cluster-size", type=int, default=5, help="the fewest images that are a cluster")
    ap.add_argument("--min-pts", type=int, default=None, help="neighbours (the image itself included) of the core similarity; default: --min-cluster-size")
    ap.add_argument("--floor", type=float, default=None, help="ignore every cosine below this")
    ap.add_argument("--selection", choices=["eom", "leaf"], default="eom")
    ap.add_argument("--allow-single-cluster", action="store_true")
    ap.add_argument("--out", required=True, help="the .npz to write")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/hdbscan.py needs a HIP device; the product path has no CPU fallback")
    from ivit_amd import cluster
    from ivit_amd.predict import hdbscan_fit
    device = "cuda:0"
    cfg, eng, s_in = build_engine(args, device)
    d = np.load(args.data)
    n = len(d["offsets"]) if "pixels" in d.files else len(d["images"])
    labels = d["labels"].astype(np.int64).reshape(-1) if "labels" in d.files else np.zeros(0, np.int64)
    mine, transform = load_share(d, labels if len(labels) else np.zeros(n, np.int64), cfg, s_in, args, device, 0, n)
    batches = (mine[a:a + args.batch] for a in range(0, n, args.batch))
    label, core, tree, condensed, _ = hdbscan_fit(eng, batches, args.min_cluster_size, args.min_pts, args.floor, args.selection,
                                                  args.allow_single_cluster, transform=transform)
    compact, count = cluster.compact_labels(label)
    out = dict(label=label.cpu().numpy(), cluster=compact.cpu().numpy(), core=core.cpu().numpy(), edge_u=tree.u.cpu().numpy(),
               edge_v=tree.v.cpu().numpy(), edge_val=tree.val.cpu().numpy(), stability=condensed.stability, birth=condensed.birth, name=condensed.name)
    line = {"n": int(n), "min_cluster_size": args.min_cluster_size, "min_pts": args.min_pts or args.min_cluster_size, "clusters": count,
            "noise_share": int((label < 0).sum()) / max(n, 1), "rounds": tree.rounds, "model": args.model, "out": args.out}
    if len(labels) and count:
        C = int(labels.max()) + 1
        table = cluster.contingency(compact, torch.from_numpy(labels).to(compact.device), count, C)      # a noise row is out of range: left out
        out["purity"], out["nmi"] = np.float64(cluster.purity(table)), np.float64(cluster.nmi(table))
        line.update(purity=float(out["purity"]), nmi=float(out["nmi"]))
    np.savez(args.out, **out)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
