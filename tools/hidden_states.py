"""Hidden states of a frozen model over a file of images: the 16-bit outputs of chosen blocks of a ViT / DeiT or of chosen stages of a
Swin — the integers of the reference's closing QuantAct of a block, qact4 — and their fp32 form, on the native engine
(NativeEngine.hidden_states, include/ivit_hidden.h).

    python tools/hidden_states.py data.npz --model deit_small --golden tests/golden/deit_small_b4.npz --blocks 3,7,11 --out hid.npz
    python tools/hidden_states.py data.npz --model swin_tiny --state-dict checkpoint.pth.tar --stages 0,1,2,3 --layout grid --out hid.npz

data.npz and the model are given as to tools/embed.py, tools/evaluate.py and tools/class_map.py (the same loading code: int8 model
inputs, uint8 [N, H, W, 3] images or a packed ragged file; --golden or --state-dict).  --blocks goes with a ViT, --stages with a Swin;
negative indices count from the end; the default is the last one.  Writes to --out, for the j-th index i of the list,
  hid16_<i>   int16 [N, T, D] (ViT, class row included) or [N, L_s, C_s] (Swin, row-major over the stage's grid)
  hid32_<i>   float32, only with --layout: "tokens" the same shape, "grid" [N, D, gh, gw] (ViT: patch rows only) or [N, C_s, res, res]
  sites       int32 [n]     the indices, ascending
  scales      float32 [n]   the per-tensor scale of every plane: hid32 = hid16 * scale, one float32 multiply
  labels      int64 [N]     copied from data.npz (empty if it has none)
Prints one JSON line {"n", "sites", "layout", "model", "out"}.  One device."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from evaluate import add_input_arguments, build_engine, load_share  # noqa: E402


def index_list(text):
    return tuple(int(t) for t in text.split(","))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    add_input_arguments(ap)
    ap.add_argument("--out", required=True, help="the .npz to write")
    which = ap.add_mutually_exclusive_group()
    which.add_argument("--blocks", type=index_list, help="a ViT's blocks, comma-separated (default: the last)")
    which.add_argument("--stages", type=index_list, help="a Swin's stages, comma-separated (default: the last)")
    ap.add_argument("--layout", choices=("tokens", "grid"), default=None, help="also write the fp32 form in this layout")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/hidden_states.py needs a HIP device; the product path has no CPU fallback")
    device = "cuda:0"
    cfg, eng, s_in = build_engine(args, device)
    swin = eng.HIDDEN_SITE == "stage"
    if (args.stages is not None and not swin) or (args.blocks is not None and swin):
        raise SystemExit(f"--model {args.model}: --blocks goes with a ViT, --stages with a Swin")
    asked = args.stages if swin else args.blocks
    sites = eng._hidden_list(asked if asked is not None else -1)
    d = np.load(args.data)
    n = len(d["offsets"]) if "pixels" in d.files else len(d["images"])
    labels = d["labels"].astype(np.int64).reshape(-1) if "labels" in d.files else np.zeros(0, np.int64)
    mine, transform = load_share(d, labels if len(labels) else np.zeros(n, np.int64), cfg, s_in, args, device, 0, n)
    parts16, parts32 = {i: [] for i in sites}, {i: [] for i in sites}
    for a in range(0, n, args.batch):
        images = mine[a:a + args.batch]
        hid16, hid32 = eng.hidden_states(transform(images) if transform is not None else images, sites, layout=args.layout)
        for j, i in enumerate(sites):
            parts16[i].append(hid16[j].cpu().numpy())
            if hid32 is not None:
                parts32[i].append(hid32[j].cpu().numpy())
    arrays = {f"hid16_{i}": np.concatenate(v) for i, v in parts16.items() if v}
    arrays.update({f"hid32_{i}": np.concatenate(v) for i, v in parts32.items() if v})
    np.savez(args.out, sites=np.asarray(sites, np.int32), scales=np.asarray([eng.hidden_scale_host(i) for i in sites], np.float32),
             labels=labels, **arrays)
    print(json.dumps({"n": int(n), "sites": list(sites), "layout": args.layout, "model": args.model, "out": args.out}))


if __name__ == "__main__":
    main()
