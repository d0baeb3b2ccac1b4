"""k-NN evaluation of a frozen backbone, the usual protocol: the gallery images' int8 features are searched for every query's k
nearest (`engine.retrieve`: the forward without the head, then ivit_search_topk of include/ivit_search.h), the neighbours vote for
their labels with weight exp(cosine / T), and top-1 / top-5 of the vote are counted against the queries' labels.

    python tools/knn.py gallery.npz queries.npz --model deit_tiny --golden tests/golden/deit_tiny_b1.npz --k 20
    python tools/knn.py gallery.npz queries.npz --model deit_small --state-dict checkpoint.pth.tar --k 200 --T 0.07 --batch 128

Both files and the model are given as to tools/embed.py (the same loading code: int8 model inputs, uint8 [N, H, W, 3] images or a
packed ragged file; --golden or --state-dict); both need `labels`.  --dot ranks by the exact integer dot product instead of the
cosine and votes with weight exp(dot * scale^2 / T).  Prints one JSON line {"n", "gallery", "k", "T", "correct", "acc", "model"}.
One device; nothing but the [B, k] neighbours leaves the search."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from evaluate import add_input_arguments, build_engine, load_share  # noqa: E402
from ivit_amd.predict import embed8, knn_evaluate  # noqa: E402
from ivit_amd.search import Gallery  # noqa: E402


def batches_of(path, cfg, s_in, args, device):
    d = np.load(path)
    if "labels" not in d.files:
        raise SystemExit(f"{path} has no labels")
    labels = d["labels"].astype(np.int64).reshape(-1)
    mine, transform = load_share(d, labels, cfg, s_in, args, device, 0, len(labels))
    share = torch.from_numpy(labels).to(device)
    return [(mine[a:a + args.batch], share[a:a + args.batch]) for a in range(0, len(labels), args.batch)], transform, labels


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    add_input_arguments(ap)                                 # `data` is the gallery
    ap.add_argument("queries")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--T", type=float, default=0.07)
    ap.add_argument("--topk", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--dot", action="store_true", help="rank by the integer dot product instead of the cosine")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/knn.py needs a HIP device; the product path has no CPU fallback")
    device = "cuda:0"
    cfg, eng, s_in = build_engine(args, device)
    gbatches, gtransform, glabels = batches_of(args.data, cfg, s_in, args, device)
    feat8, scale = embed8(eng, gbatches, transform=gtransform)
    gallery = Gallery(feat8, labels=glabels, cosine=not args.dot)
    qbatches, qtransform, _ = batches_of(args.queries, cfg, s_in, args, device)
    T = args.T if not args.dot else args.T / (scale * scale)           # a dot product of integers is scale^-2 times that of the features
    out = knn_evaluate(eng, gallery, qbatches, k=min(args.k, gallery.rows), T=T, topk=args.topk, transform=qtransform)
    print(json.dumps({"n": out["n"], "gallery": gallery.rows, "k": min(args.k, gallery.rows), "T": args.T, "dot": bool(args.dot),
                      "correct": {str(j): c for j, c in out["correct"].items()}, "acc": {str(j): a for j, a in out["acc"].items()},
                      "model": args.model}))


if __name__ == "__main__":
    main()
