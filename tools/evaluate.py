"""Top-k accuracy of a frozen model over a file of images and labels: the counterpart of the reference's
`quant_train.py --evaluate` (validate(), quant_train.py:314-351) without its data loader.

    python tools/evaluate.py data.npz --model deit_tiny --golden tests/golden/deit_tiny_b1.npz
    python tools/evaluate.py data.npz --model deit_small --state-dict checkpoint.pth.tar --batch 128 --topk 1 5

data.npz holds `images` and `labels` [N].  images uint8 [N, H, W, 3]: raw pixels, taken through the reference's eval transform on
the device (resize --resize, centre crop to the model's input, normalise, input QuantAct).  images int8 [N, C, S, S]: already
quantised at the model's input scale, fed as they are.
The model is a name from ivit_amd.CONFIGS / SWIN_CONFIGS with either
  --golden F      the seeded synthetic weights and the calibrated scales recorded in a tests/golden fixture, or
  --state-dict F  a reference state dict / checkpoint (float parameters and act_scaling_factor buffers; ivit_amd.checkpoint).
Prints one JSON line {"n", "correct", "acc", "model", "batch"}; under torch.distributed.run every rank evaluates its shard of the
file and rank 0 prints the reduced result (IVIT_DIST_BACKEND picks the backend, as in bench.py)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ivit_amd as iv  # noqa: E402
from ivit_amd import dist as ivdist  # noqa: E402
from ivit_amd.predict import evaluate  # noqa: E402


def build_engine(args, device):
    swin = args.model in iv.SWIN_CONFIGS
    cfg = (iv.SWIN_CONFIGS if swin else iv.CONFIGS)[args.model]
    if args.state_dict:
        from ivit_amd.checkpoint import split_state_dict
        weights, scales, _ = split_state_dict(args.state_dict)
    else:
        g = np.load(args.golden)
        if str(g["cfg_name"]) != args.model:
            raise SystemExit(f"{args.golden} was recorded for {g['cfg_name']}, not {args.model}")
        scales = {k[len("scale/"):]: np.float32(g[k]) for k in g.files if k.startswith("scale/")}
        weights = (iv.make_swin_weights if swin else iv.make_vit_weights)(cfg, int(g["seed"]))
    if swin:
        from ivit_amd.swin_engine import SwinEngine
        return cfg, SwinEngine(cfg, weights, scales, device=device), np.float32(scales["qact_input"])
    from ivit_amd.engine import ViTEngine
    return cfg, ViTEngine.from_float(cfg, weights, scales, device=device), np.float32(scales["qact_input"])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("data")
    ap.add_argument("--model", required=True)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--golden")
    src.add_argument("--state-dict")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--topk", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--resize", type=int, default=0, help="shorter side before the centre crop (default: int(crop / 0.875))")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/evaluate.py needs a HIP device; the product path has no CPU fallback")
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count()
    torch.cuda.set_device(local)
    device = f"cuda:{local}"
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group(os.environ.get("IVIT_DIST_BACKEND", "nccl"), rank=rank, world_size=world)
    cfg, eng, s_in = build_engine(args, device)
    d = np.load(args.data)
    images, labels = d["images"], d["labels"].astype(np.int64).reshape(-1)
    if len(images) != len(labels):
        raise SystemExit(f"{len(images)} images but {len(labels)} labels")
    transform = None
    if images.dtype == np.uint8 and images.ndim == 4 and images.shape[-1] == 3:
        from ivit_amd.preprocess import eval_transform
        size = args.resize or int(cfg.img_size / 0.875)
        transform = lambda u8: eval_transform(u8, s_in, size, cfg.img_size)      # noqa: E731
    elif not (images.dtype == np.int8 and images.shape[1:] == (cfg.in_chans, cfg.img_size, cfg.img_size)):
        raise SystemExit(f"images must be uint8 [N, H, W, 3] or int8 [N, {cfg.in_chans}, {cfg.img_size}, {cfg.img_size}]; "
                         f"got {images.dtype} {images.shape}")
    lo, hi = ivdist.shard_range(len(labels), rank, world)
    mine = torch.from_numpy(np.ascontiguousarray(images[lo:hi])).to(device)      # this rank's share only
    share = torch.from_numpy(labels[lo:hi]).to(device)                           # once: no copy inside evaluate's loop
    batches = ((mine[a:a + args.batch], share[a:a + args.batch]) for a in range(0, hi - lo, args.batch))
    out = evaluate(eng, batches, topk=args.topk, transform=transform, rank=rank, world=world)       # ends with the one all_reduce
    if rank == 0:
        print(json.dumps({"n": out["n"], "correct": {str(j): c for j, c in out["correct"].items()},
                          "acc": {str(j): a for j, a in out["acc"].items()}, "model": args.model, "batch": args.batch, "ranks": world}))
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
