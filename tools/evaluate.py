"""Top-k accuracy — and with --loss the cross-entropy — of a frozen model over a file of images and labels: the counterpart of
the reference's `quant_train.py --evaluate` (validate(), quant_train.py:314-351) without its data loader.

    python tools/evaluate.py data.npz --model deit_tiny --golden tests/golden/deit_tiny_b1.npz
    python tools/evaluate.py data.npz --model deit_tiny --golden tests/golden/deit_tiny_b1.npz --loss
    python tools/evaluate.py data.npz --model deit_small --state-dict checkpoint.pth.tar --batch 128 --topk 1 5

data.npz holds `labels` [N] and the images in one of three forms:
  images uint8 [N, H, W, 3]   raw pixels of one size, taken through the reference's eval transform on the device (resize --resize,
                              centre crop to the model's input, normalise, input QuantAct).  --resample torch (the default) is the
                              torch-pinned transform (ivit_amd.preprocess.eval_transform), --resample pil the PIL-exact one;
  pixels uint8 [total], offsets int64 [N], shapes int32 [N, 2]
                              raw pixels of DIFFERENT sizes, image i = shapes[i] = (h, w) HWC at pixels[offsets[i]:].  The buffer
                              is uploaded once per rank and every batch is one launch of eval_transform_pil: the bytes PIL hands
                              the reference (utils/data_utils.py:82-92), so the count is the one `quant_train.py --evaluate` gives;
  images int8 [N, C, S, S]    already quantised at the model's input scale, fed as they are.
With --jpeg-dir DIR the file holds `labels` [N] and `files` [N], names of JPEG files under DIR: every batch is decoded by
ivit_amd.jpeg.decode (entropy decode on --jpeg-threads host threads, reconstruction on the device: Pillow's bytes; files the decoder
refuses go through Pillow) and taken through eval_transform_pil, so the count is again the one `quant_train.py --evaluate` gives.
The model is a name from ivit_amd.CONFIGS / SWIN_CONFIGS with either
  --golden F      the seeded synthetic weights and the calibrated scales recorded in a tests/golden fixture, or
  --state-dict F  a reference state dict / checkpoint (float parameters and act_scaling_factor buffers; ivit_amd.checkpoint).
Or, in place of --model and its source, --model-file F: a frozen model file written by tools/freeze.py or `engine.save`
(include/ivit_modelfile.h); nothing is frozen again, the input scale comes from the file, "model" is the file's configuration name.
Prints one JSON line {"n", "correct", "acc", "model", "batch"}; under torch.distributed.run every rank evaluates its shard of the
file and rank 0 prints the reduced result (IVIT_DIST_BACKEND picks the backend, as in bench.py).
--loss scores every image on the device (ivit_amd.predict.evaluate(loss=True): rank and negative log-likelihood of the label, any
--topk, no limit of 16), adds "loss" to the JSON line and prints validate()'s summary after it, ` * Loss 6.9078e+00 Prec@1 0.100
Prec@5 0.500` (the loss as its meter formats it, quant_train.py:316; a Prec@j per --topk entry).  Without --loss the output is
unchanged.
--views 5 / --views 10 (ragged files and --resample pil): five-crop / ten-crop evaluation — the corners and the centre of the resized
image, and with 10 the same of its mirror image (ivit_amd.views), all views of a batch in one launch, predictions and loss of the
MEAN logits of every image's views (ivit_amd.predict.evaluate(views=)).  --batch still names the images a forward sees: a batch
holds max(1, batch // views) images.  Adds "views" to the JSON line."""
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
    if args.model_file:
        if args.model:
            raise SystemExit("--model-file holds the model: give it without --model")
        import ivit_amd.model_file as mf
        try:
            eng = mf.load_engine(args.model_file, device=device)
        except mf.ModelFileError as e:
            raise SystemExit(f"{args.model_file}: {e}")
        args.model = eng.cfg.name
        return eng.cfg, eng, np.float32(eng.input_scale_host())
    if not args.model:
        raise SystemExit("--model NAME is required with --golden / --state-dict")
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


def add_input_arguments(ap):
    """the data file, the model and its source, the batch and the resize: what tools/embed.py takes too"""
    ap.add_argument("data")
    ap.add_argument("--model", help="a name from CONFIGS / SWIN_CONFIGS, with --golden or --state-dict")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--golden")
    src.add_argument("--state-dict")
    src.add_argument("--model-file", help="a frozen model file (tools/freeze.py, engine.save) in place of --model and its source")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--resize", type=int, default=0, help="shorter side before the centre crop (default: int(crop / 0.875))")
    ap.add_argument("--resample", choices=("torch", "pil"), default="torch",
                    help="uint8 [N, H, W, 3] images: the torch-pinned resize (default) or the PIL-exact one; ragged files are always pil")


def load_share(d, labels, cfg, s_in, args, device, lo, hi):
    """images lo .. hi of the opened data file `d` in any of its three forms, uploaded once -> (what batches are sliced from,
    the transform that turns a slice into the engine's int8 input, or None)"""
    size = args.resize or int(cfg.img_size / 0.875)
    transform = None
    if getattr(args, "jpeg_dir", None):
        from ivit_amd.jpeg import decode
        from ivit_amd.preprocess import eval_transform_pil
        if "files" not in d.files or len(d["files"]) != len(labels):
            raise SystemExit("--jpeg-dir needs `files` [N] beside `labels` [N]")
        if getattr(args, "views", 1) != 1:
            raise SystemExit("--views is not available with --jpeg-dir")
        mine = [os.path.join(args.jpeg_dir, str(f)) for f in d["files"][lo:hi]]
        return mine, lambda paths: eval_transform_pil(decode(paths, device, threads=args.jpeg_threads)[0], s_in, size, cfg.img_size)
    if "pixels" in d.files or (args.resample == "pil" and d["images"].dtype == np.uint8):
        from ivit_amd.preprocess import DESC_DTYPE, RaggedImages, eval_transform_pil
        if "pixels" in d.files:
            pixels, offsets, shapes = d["pixels"], d["offsets"].astype(np.int64).reshape(-1), d["shapes"].astype(np.int64).reshape(-1, 2)
        else:                                                                    # equal sizes, described as a ragged batch
            images = d["images"]
            if images.ndim != 4 or images.shape[-1] != 3:
                raise SystemExit(f"images must be uint8 [N, H, W, 3]; got {images.shape}")
            pixels = images.reshape(-1)
            shapes = np.tile(np.array(images.shape[1:3], np.int64), (len(images), 1))
            offsets = np.arange(len(images), dtype=np.int64) * int(np.prod(images.shape[1:]))
        if pixels.dtype != np.uint8 or not (len(offsets) == len(shapes) == len(labels)):
            raise SystemExit(f"pixels must be uint8 and offsets, shapes, labels of one length; got {pixels.dtype}, "
                             f"{len(offsets)}, {len(shapes)}, {len(labels)}")
        ends = offsets + shapes[:, 0] * shapes[:, 1] * 3
        if (shapes < 1).any() or (offsets < 0).any() or (ends > pixels.size).any():
            raise SystemExit("an image record lies outside `pixels`")
        # this rank's share of the packed buffer only, uploaded once; offsets relative to it
        first, last = (int(offsets[lo:hi].min()), int(ends[lo:hi].max())) if hi > lo else (0, 0)
        desc = np.zeros(hi - lo, DESC_DTYPE)
        desc["offset"], desc["h"], desc["w"] = offsets[lo:hi] - first, shapes[lo:hi, 0], shapes[lo:hi, 1]
        mine = RaggedImages(torch.from_numpy(np.ascontiguousarray(pixels[first:last])).to(device), desc)
        nviews = getattr(args, "views", 1)
        if nviews == 1:
            transform = lambda rag: eval_transform_pil(rag, s_in, size, cfg.img_size)      # noqa: E731
        else:
            from ivit_amd import views as vw
            table = vw.five_crop_views if nviews == 5 else vw.ten_crop_views
            transform = lambda rag: vw.view_transform(rag, table(rag, size, cfg.img_size), s_in, cfg.img_size)      # noqa: E731
    else:
        images = d["images"]
        if len(images) != len(labels):
            raise SystemExit(f"{len(images)} images but {len(labels)} labels")
        if images.dtype == np.uint8 and images.ndim == 4 and images.shape[-1] == 3:
            from ivit_amd.preprocess import eval_transform
            transform = lambda u8: eval_transform(u8, s_in, size, cfg.img_size)      # noqa: E731
        elif not (images.dtype == np.int8 and images.shape[1:] == (cfg.in_chans, cfg.img_size, cfg.img_size)):
            raise SystemExit(f"images must be uint8 [N, H, W, 3] or int8 [N, {cfg.in_chans}, {cfg.img_size}, {cfg.img_size}]; "
                             f"got {images.dtype} {images.shape}")
        if getattr(args, "views", 1) != 1:
            raise SystemExit("--views needs raw pixels on the PIL-exact path: a ragged file, or uint8 images with --resample pil")
        mine = torch.from_numpy(np.ascontiguousarray(images[lo:hi])).to(device)      # this rank's share only
    return mine, transform


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    add_input_arguments(ap)
    ap.add_argument("--topk", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--loss", action="store_true", help="also the mean cross-entropy of the labels (validate()'s Loss), computed on the device")
    ap.add_argument("--views", type=int, choices=(1, 5, 10), default=1,
                    help="views per image: 1 the centre crop (default), 5 five-crop, 10 ten-crop; the mean logits are scored")
    ap.add_argument("--jpeg-dir", help="`files` of the data file are JPEG files under this directory, decoded by ivit_amd.jpeg.decode")
    ap.add_argument("--jpeg-threads", type=int, default=8, help="host threads of the entropy decode (at most 16)")
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
    labels = d["labels"].astype(np.int64).reshape(-1)
    lo, hi = ivdist.shard_range(len(labels), rank, world)
    share = torch.from_numpy(labels[lo:hi]).to(device)                           # once: no copy inside evaluate's loop
    mine, transform = load_share(d, labels, cfg, s_in, args, device, lo, hi)
    step = max(1, args.batch // args.views)                                      # a forward still sees about --batch images
    batches = ((mine[a:a + step], share[a:a + step]) for a in range(0, hi - lo, step))
    out = evaluate(eng, batches, topk=args.topk, transform=transform, rank=rank, world=world, loss=args.loss, views=args.views)     # ends with the one all_reduce
    if rank == 0:
        print(json.dumps({"n": out["n"], "correct": {str(j): c for j, c in out["correct"].items()},
                          "acc": {str(j): a for j, a in out["acc"].items()}, "model": args.model, "batch": args.batch, "ranks": world,
                          **({"views": args.views} if args.views != 1 else {}), **({"loss": out["loss"]} if args.loss else {})}))
        if args.loss:
            print(" * Loss {:.4e} ".format(out["loss"]) + " ".join("Prec@{} {:.3f}".format(j, a) for j, a in out["acc"].items()))
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
