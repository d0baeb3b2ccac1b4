"""The single-linkage hierarchy of a frozen model's int8 features over a file of images (include/ivit_linkage.h, ivit_amd/cluster.py):
one tree that answers every similarity threshold, for choosing the threshold of tools/dedup.py and tools/dbscan.py.

    python tools/linkage.py data.npz --model-file deit_small.ivit [--floor 0.5] [--cut 0.9 | --clusters 20] --out tree.npz

data.npz and the model are given as to tools/kmeans.py (the same loading code).  The images are embedded once
(`predict.linkage_fit`: the int8 features of the dataset are kept on the device), then the maximum-cosine spanning forest of their
features is built on the device; --floor leaves out every pair below it (default: none, a tree of N - 1 edges).  Writes to --out
  u, v       int32 [E]      the edges, u < v, in the edge order (val descending, then u, then v)
  val        float32 [E]    their cosines: cutting at t keeps the edges with val >= t
  Z          float64 [E, 4] the linkage matrix in SciPy's convention, distance -val
  group      int64 [N]      with --cut T: the smallest image of every image's component at a cosine >= T (what tools/dedup.py
                            keeps one of); with --clusters K: the same after removing the K - 1 weakest edges
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
    ap.add_argument("--floor", type=float, default=None, help="leave out every pair whose cosine is below this")
    how = ap.add_mutually_exclusive_group()
    how.add_argument("--cut", type=float, default=None, help="also write the groups at this cosine")
    how.add_argument("--clusters", type=int, default=None, help="also write the groups after removing the K - 1 weakest edges")
    ap.add_argument("--out", required=True, help="the .npz to write")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/linkage.py needs a HIP device; the product path has no CPU fallback")
    from ivit_amd.predict import linkage_fit
    device = "cuda:0"
    cfg, eng, s_in = build_engine(args, device)
    d = np.load(args.data)
    n = len(d["offsets"]) if "pixels" in d.files else len(d["images"])
    mine, transform = load_share(d, np.zeros(n, np.int64), cfg, s_in, args, device, 0, n)
    batches = (mine[a:a + args.batch] for a in range(0, n, args.batch))
    tree, _ = linkage_fit(eng, batches, floor=args.floor, transform=transform)
    out = dict(u=tree.u.cpu().numpy(), v=tree.v.cpu().numpy(), val=tree.val.cpu().numpy(), Z=tree.matrix())
    line = {"n": int(n), "edges": int(tree.u.shape[0]), "rounds": tree.rounds, "floor": args.floor, "model": args.model, "out": args.out}
    if args.cut is not None or args.clusters is not None:
        out["group"] = tree.cut(args.cut) if args.cut is not None else tree.cut_k(args.clusters)
        line["groups"] = int(len(np.unique(out["group"])))
    np.savez(args.out, **out)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
