"""Near-duplicates of a file of images by a frozen model's int8 features, exact (include/ivit_range.h, ivit_amd/search.py).

    python tools/dedup.py data.npz --model-file deit_small.ivit --threshold 0.95 --out dups.npz
    python tools/dedup.py val.npz --model-file deit_small.ivit --threshold 0.95 --against train.npz --out leaks.npz
    python tools/dedup.py data.npz --model deit_tiny --golden tests/golden/deit_tiny_b1.npz --threshold 4000 --dot --out dups.npz

data.npz and the model are given as to tools/embed.py (the same loading code).  The images are embedded once (`predict.embed8`: the
int8 features of the dataset are kept on the device) and joined with themselves by the triangle self-join (`search.duplicates`):
every pair i < j whose cosine — with --dot the exact integer dot product — is >= --threshold, as `predict.range_reference` states
it; the [N, N] matrix is never written.  Writes to --out
  pairs      int64 [P, 2]               i < j, in lexicographic order
  val        float32 [P]                the cosine (dot product) of every pair
  group      int64 [N]                  for every image the smallest index of its connected component (`search.duplicate_groups`)
  keep       bool [N]                   group == arange(N): one image per component, the deduplicated subset
  scale      float32                    the features' scale
With --against other.npz the join is between the two files instead (`search.cross_matches`: the leakage check): pairs holds (i in
data.npz, j in other.npz), val their values, and group / keep are not written.  Prints one JSON line.  One device."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from evaluate import add_input_arguments, build_engine, load_share  # noqa: E402


def embed_file(path, eng, cfg, s_in, args, device):
    """(feat8 int8 [N, num_features] on the device, N) of the images of one data file"""
    from ivit_amd.predict import embed8
    d = np.load(path)
    n = len(d["offsets"]) if "pixels" in d.files else len(d["images"])
    mine, transform = load_share(d, np.zeros(n, np.int64), cfg, s_in, args, device, 0, n)
    return embed8(eng, (mine[a:a + args.batch] for a in range(0, n, args.batch)), transform)[0], n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    add_input_arguments(ap)
    ap.add_argument("--threshold", type=float, required=True, help="cosine (with --dot: integer dot product) a pair must reach")
    ap.add_argument("--against", default=None, help="a second data file: the matches between the two instead of the self-join")
    ap.add_argument("--dot", action="store_true", help="the exact integer dot product instead of the cosine")
    ap.add_argument("--chunk-rows", type=int, default=None, help="join in chunks of this many rows (the result does not depend on it)")
    ap.add_argument("--out", required=True, help="the .npz to write")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/dedup.py needs a HIP device; the product path has no CPU fallback")
    from ivit_amd import search
    device = "cuda:0"
    cfg, eng, s_in = build_engine(args, device)
    feat8, n = embed_file(args.data, eng, cfg, s_in, args, device)
    out = dict(scale=np.float32(eng.feature_scale_host()))
    line = {"n": int(n), "threshold": args.threshold, "cosine": not args.dot, "model": args.model, "out": args.out}
    if args.against:
        other8, m = embed_file(args.against, eng, cfg, s_in, args, device)
        pairs, val = search.cross_matches(feat8, other8, args.threshold, cosine=not args.dot, chunk_rows=args.chunk_rows)
        line.update(against=args.against, m=int(m), leaked=int(torch.unique(pairs[:, 0]).numel()))
    else:
        pairs, val = search.duplicates(feat8, args.threshold, cosine=not args.dot, chunk_rows=args.chunk_rows)
        group = search.duplicate_groups(pairs, n)
        out.update(group=group, keep=group == np.arange(n))
        line.update(kept=int(out["keep"].sum()))
    out.update(pairs=pairs.cpu().numpy(), val=val.cpu().numpy())
    line.update(pairs=int(out["pairs"].shape[0]))
    np.savez(args.out, **out)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
