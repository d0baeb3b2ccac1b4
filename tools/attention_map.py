"""Class-token attention maps of a frozen ViT / DeiT over a file of images: row 0 of IntSoftmax's output (vit_quant.py:76) of the
blocks asked for, on the native engine (ViTEngine.attention, include/ivit_attnmap.h).

    python tools/attention_map.py data.npz --model deit_tiny --golden tests/golden/deit_tiny_b1.npz --blocks -1 --out maps.npz
    python tools/attention_map.py data.npz --model deit_small --state-dict checkpoint.pth.tar --blocks 0 5 11 --heads --topk 5 --out maps.npz

data.npz and the model are given as to tools/embed.py and tools/evaluate.py (the same loading code: int8 model inputs, uint8
[N, H, W, 3] images or a packed ragged file; --golden or --state-dict); `labels` is optional.  --blocks: block indices, negative ones
counting from the end, strictly ascending after that.  Writes to --out
  blocks    int64 [n]                        the blocks, as non-negative indices
  attn16    uint16 [n, N, heads, T]          the class token's attention probabilities, the reference's integers, scale 2^-15
  maps      float32 [n, N, gh, gw]           their patch columns on the patch grid, the mean over the heads — or with --heads
            float32 [n, N, heads, gh, gw]    each head's own (attn16 * 2^-15)
  labels    int64 [N]                        copied from data.npz (empty if it has none)
and with --topk K also  topk_idx int32 [N, K], topk_val float32 [N, K]: the predictions, from the same forward as the maps.
Prints one JSON line {"n", "blocks", "heads", "grid", "model", "out"}.  One device.  A Swin has no class token: ViT / DeiT only."""
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
    ap.add_argument("--blocks", type=int, nargs="+", default=[-1], help="block indices (negative: from the end), ascending; default: the last")
    ap.add_argument("--heads", action="store_true", help="one map per head instead of their mean")
    ap.add_argument("--topk", type=int, default=0, help="also write the K best classes of every image and their values")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/attention_map.py needs a HIP device; the product path has no CPU fallback")
    device = "cuda:0"
    cfg, eng, s_in = build_engine(args, device)
    if not hasattr(eng, "attention"):
        raise SystemExit(f"--model {args.model}: attention maps are a ViT / DeiT feature (a Swin has no class token)")
    from ivit_amd.predict import topk_reference
    blocks = eng._attention_blocks(args.blocks)             # ValueError on a bad list, before any image is read
    d = np.load(args.data)
    n = len(d["offsets"]) if "pixels" in d.files else len(d["images"])
    labels = d["labels"].astype(np.int64).reshape(-1) if "labels" in d.files else np.zeros(0, np.int64)
    mine, transform = load_share(d, labels if len(labels) else np.zeros(n, np.int64), cfg, s_in, args, device, 0, n)
    attn16, maps, logits = [], [], []
    for a in range(0, n, args.batch):
        images = mine[a:a + args.batch]
        out = eng.attention(transform(images) if transform is not None else images, blocks=blocks, heads=args.heads,
                            logits=args.topk > 0, copy=True)
        attn16.append(out[0].cpu().numpy())
        maps.append(out[1].cpu().numpy())
        if args.topk > 0:
            logits.append(out[2].cpu().numpy())
    g = cfg.img_size // cfg.patch_size
    nb, H, T = len(blocks), cfg.num_heads, cfg.num_tokens
    attn16 = np.concatenate(attn16, axis=1) if attn16 else np.zeros((nb, 0, H, T), np.uint16)
    maps = np.concatenate(maps, axis=1) if maps else np.zeros((nb, 0, H, g, g) if args.heads else (nb, 0, g, g), np.float32)
    extra = {}
    if args.topk > 0:
        acc = np.concatenate(logits) if logits else np.zeros((0, cfg.num_classes), np.int32)
        extra["topk_idx"], extra["topk_val"] = topk_reference(acc, eng.head_scale_host(), args.topk) if len(acc) else (
            np.zeros((0, args.topk), np.int32), np.zeros((0, args.topk), np.float32))
    np.savez(args.out, blocks=np.asarray(blocks, np.int64), attn16=attn16, maps=maps, labels=labels, **extra)
    print(json.dumps({"n": int(n), "blocks": list(blocks), "heads": bool(args.heads), "grid": [g, g], "model": args.model, "out": args.out}))


if __name__ == "__main__":
    main()
