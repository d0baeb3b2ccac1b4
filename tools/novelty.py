"""Novelty scores on a frozen backbone, from a file of labelled training images to AUROC: one pass over the training images
(engine.probe_accumulate: the Gaussian model's sufficient statistics, no feature stored), the fit on the host (ivit_amd.gauss.fit), then
engine.novelty (features without the head, then ivit_gauss_score) over a file of inliers and a file of outliers.

    python tools/novelty.py train.npz --model-file deit_small.ivit --classes 10 --inliers val.npz --outliers other.npz
    python tools/novelty.py train.npz --model-file deit_small.ivit --classes 10 --inliers val.npz --outliers other.npz --rank 128 --out scores.npz

train.npz, the other two files and the model are given as to tools/probe.py (the same loading code); `labels` [N] of train.npz are the
classes, a label outside 0 .. --classes - 1 is ignored; the inliers' labels are compared with the model's class (the equal-prior LDA
prediction), the outliers' are not used.  Prints one JSON line {"n", "used", "classes", "rank", "shrinkage", "inliers", "outliers",
"auroc", "fpr_at_95_tpr", "lda_acc", "model"}; --out F also writes dist and cls of both files (and the model's four arrays).  One
device."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from evaluate import add_input_arguments, build_engine  # noqa: E402
from probe import batches_of  # noqa: E402
from ivit_amd import gauss  # noqa: E402
from ivit_amd.probe import ProbeStats  # noqa: E402


def scores_of(path, eng, model, cfg, s_in, args, device):
    """(dist float32 [n], cls int32 [n], labels int64 [n]) of a data file"""
    batches, transform, _ = batches_of(path, cfg, s_in, args, device)
    dist, cls, labels = [], [], []
    for images, lab in batches:
        d, c, _ = eng.novelty(transform(images) if transform is not None else images, model)
        dist.append(d)
        cls.append(c)
        labels.append(lab)
    return tuple(torch.cat(t).cpu().numpy() for t in (dist, cls, labels))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    add_input_arguments(ap)
    ap.add_argument("--classes", type=int, required=True, help="number of classes of train.npz")
    ap.add_argument("--inliers", required=True, help="a data file like the training data")
    ap.add_argument("--outliers", required=True, help="a data file unlike it")
    ap.add_argument("--rank", type=int, help="a multiple of 32: the distance in the leading principal subspace (default: all features)")
    ap.add_argument("--shrinkage", type=float, default=1e-3, help="of the covariance towards its mean variance")
    ap.add_argument("--out", help="an .npz file for the scores")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/novelty.py needs a HIP device; the product path has no CPU fallback")
    device = "cuda:0"
    cfg, eng, s_in = build_engine(args, device)
    batches, transform, n = batches_of(args.data, cfg, s_in, args, device)
    stats = ProbeStats(eng.num_features, args.classes, device)
    for images, labels in batches:
        eng.probe_accumulate(transform(images) if transform is not None else images, labels, stats)
    model = gauss.fit(stats, args.shrinkage, args.rank)
    d_in, c_in, lab = scores_of(args.inliers, eng, model, cfg, s_in, args, device)
    d_out, c_out, _ = scores_of(args.outliers, eng, model, cfg, s_in, args, device)
    print(json.dumps({"n": int(n), "used": int(stats.count.sum().item()), "classes": int(args.classes), "rank": model.R, "shrinkage": args.shrinkage,
                      "inliers": len(d_in), "outliers": len(d_out), "auroc": gauss.auroc(d_in, d_out),
                      "fpr_at_95_tpr": gauss.fpr_at_tpr(d_in, d_out, 0.95), "lda_acc": float((c_in == lab).mean()), "model": args.model}))
    if args.out:
        np.savez(args.out, dist_inliers=d_in, cls_inliers=c_in, dist_outliers=d_out, cls_outliers=c_out, Wh=model.Wh, t=model.t, Wc=model.Wc,
                 bc=model.bc)


if __name__ == "__main__":
    main()
