"""A linear probe on a frozen backbone, from a file of labelled images to a model file with the new head: one pass over the images
(engine.probe_accumulate: features without the head, then ivit_probe_accumulate — no feature is stored), the least-squares (ridge)
fit of the new classes on the host (ivit_amd.probe.fit), `engine.with_head`, `save`.

    python tools/probe.py train.npz --model deit_tiny --golden tests/golden/deit_tiny_b1.npz --classes 37 --out pets.ivit
    python tools/probe.py train.npz --model-file deit_small.ivit --classes 10 --out new.ivit --ridge 1e-2 --eval val.npz

train.npz and the model are given as to tools/embed.py and tools/evaluate.py (the same loading code: int8 model inputs, uint8
[N, H, W, 3] images or a packed ragged file; --golden, --state-dict or --model-file); `labels` [N] are the NEW classes, a label outside
0 .. --classes - 1 is ignored.  Writes the model file --out (include/ivit_modelfile.h: what `ivit_amd.load_engine`, `ivit_model_open`
and examples/classify read) and prints one JSON line {"n", "used", "classes", "ridge", "model", "out"}; with --eval F also
tools/evaluate.py's line for the new engine over F.  One device."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from evaluate import add_input_arguments, build_engine, load_share  # noqa: E402
from ivit_amd.predict import evaluate, probe_fit  # noqa: E402
from ivit_amd.probe import ProbeStats  # noqa: E402


def batches_of(path, cfg, s_in, args, device):
    """((images, labels) batches, transform, n) of a data file"""
    d = np.load(path)
    labels = d["labels"].astype(np.int64).reshape(-1)
    n = len(labels)
    share = torch.from_numpy(labels).to(device)                   # once: no copy inside the loop
    mine, transform = load_share(d, labels, cfg, s_in, args, device, 0, n)
    return ((mine[a:a + args.batch], share[a:a + args.batch]) for a in range(0, n, args.batch)), transform, n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    add_input_arguments(ap)
    ap.add_argument("--classes", type=int, required=True, help="number of new classes")
    ap.add_argument("--out", required=True, help="the model file to write")
    ap.add_argument("--ridge", type=float, default=1e-3, help="relative to the mean feature variance")
    ap.add_argument("--eval", help="a data file to evaluate the new engine on")
    ap.add_argument("--topk", type=int, nargs="+", default=[1, 5])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/probe.py needs a HIP device; the product path has no CPU fallback")
    device = "cuda:0"
    cfg, eng, s_in = build_engine(args, device)
    batches, transform, n = batches_of(args.data, cfg, s_in, args, device)
    stats = ProbeStats(eng.num_features, args.classes, device)
    head = probe_fit(eng, batches, args.classes, ridge=args.ridge, transform=transform, stats=stats)
    new = eng.with_head(head)
    new.save(args.out)
    print(json.dumps({"n": int(n), "used": int(stats.count.sum().item()), "classes": int(args.classes), "ridge": args.ridge, "model": args.model,
                      "out": args.out}))
    if args.eval:
        batches, transform, _ = batches_of(args.eval, cfg, s_in, args, device)
        out = evaluate(new, batches, topk=args.topk, transform=transform)
        print(json.dumps({"n": out["n"], "correct": {str(j): c for j, c in out["correct"].items()},
                          "acc": {str(j): a for j, a in out["acc"].items()}, "model": args.model, "batch": args.batch, "ranks": 1}))


if __name__ == "__main__":
    main()
