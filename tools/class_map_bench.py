"""Timing of a Swin's class-activation maps on the device (profiles/README.md, "Class-activation maps"): Swin-T batch 256,
engine.class_map(k=5) — the forward with the token store, the top-k and the map launch — beside engine.predict(k=5) and
engine.forward, and with --parent DIR beside predict and forward of ANOTHER checkout's package and library (the parent commit, built
in DIR) in the same process on the same images; and the map launch alone (ivit_class_map on 256 x 5 classes, L = 49, C = 768).
The method is tools/topk_bench.py's: the variants alternate inside one loop, HIP-event times, medians with quartiles and extremes,
differences taken round by round.  Prints one JSON line per measurement.
    python tools/class_map_bench.py [--reps 100] [--parent /path/to/parent/checkout]"""
import argparse
import ctypes
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from ivit_amd.predict import class_map_reference  # noqa: E402
from topk_bench import interleaved, spread  # noqa: E402

_P = ctypes.c_void_p


def load_package(root, name):
    """the package of another checkout under another module name, bound to that checkout's own library"""
    pkg = os.path.join(root, "i-vit_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def bench_operator(reps):
    H = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    B, L, C, k, ncls = 256, 49, 768, 5, 1000
    rng = np.random.default_rng(0)
    tok8 = rng.integers(-128, 128, size=(B, L, C), dtype=np.int64).astype(np.int8)
    head_w = rng.integers(-127, 128, size=(ncls, C), dtype=np.int64).astype(np.int8)
    idx = rng.integers(0, ncls, size=(B, k), dtype=np.int64).astype(np.int32)
    scale = rng.uniform(1e-5, 1e-4, size=ncls).astype(np.float32)
    d = [torch.from_numpy(a).cuda() for a in (tok8, head_w, idx, scale)]
    cam = torch.empty(B, k, L, dtype=torch.int32, device="cuda")
    m32 = torch.empty(B, k, L, dtype=torch.float32, device="cuda")
    p = [_P(t.data_ptr()) for t in d]
    both = lambda: H.call("ivit_class_map", p[0], p[1], p[2], B, L, C, ncls, k, p[3], _P(cam.data_ptr()), _P(m32.data_ptr()))      # noqa: E731
    ints = lambda: H.call("ivit_class_map", p[0], p[1], p[2], B, L, C, ncls, k, None, _P(cam.data_ptr()), None)                      # noqa: E731
    both()
    torch.cuda.synchronize()
    want_cam, want_map = class_map_reference(tok8, head_w, idx, scale)
    same = bool(np.array_equal(cam.cpu().numpy(), want_cam)) and bool(np.array_equal(m32.cpu().numpy().view(np.uint32), want_map.view(np.uint32)))
    variants = {"cam32_and_map32": both, "cam32_only": ints}
    print(json.dumps({"what": "class-map launch", "shape": {"B": B, "k": k, "L": L, "C": C, "num_classes": ncls},
                      "single_call_us": interleaved(variants, reps)[0],
                      "train_of_20_us_per_call": interleaved(variants, max(20, reps // 4), train=20)[0],
                      "equal_to_reference": same, "cam32_sample": cam[0, 0, :4].cpu().tolist(), "reference_sample": want_cam[0, 0, :4].tolist()}),
          flush=True)


def bench_model(name, golden, B, reps, nslices, parent):
    g = np.load(os.path.join(ROOT, "tests", "golden", golden))
    cfg = iv.SWIN_CONFIGS[name]
    scales = {k[len("scale/"):]: np.float32(g[k]) for k in g.files if k.startswith("scale/")}
    from ivit_amd.swin_engine import SwinEngine
    weights = iv.make_swin_weights(cfg, int(g["seed"]))
    eng = SwinEngine(cfg, weights, scales)
    imgs = torch.from_numpy(iv.make_images_int8(cfg, B, seed=101)).cuda()
    labels = torch.zeros(B, 1, dtype=torch.int32, device="cuda")
    variants = {"forward": lambda: eng.forward(imgs, nslices=nslices),
                "predict": lambda: eng.predict(imgs, k=5, nslices=nslices),
                "class_map": lambda: eng.class_map(imgs, k=5, nslices=nslices),
                "class_map_given_headless": lambda: eng.class_map(imgs, classes=labels, logits=False, nslices=nslices)}
    fwd = eng.forward(imgs, nslices=nslices, copy=True)
    pred = eng.predict(imgs, k=5, nslices=nslices, copy=True)
    idx, val, tok8, cam32, maps = eng.class_map(imgs, k=5, nslices=nslices, copy=True)
    same = bool(torch.equal(eng.last_logits, fwd)) and bool(torch.equal(idx, pred[0])) and bool(torch.equal(val.view(torch.int32), pred[1].view(torch.int32)))
    o, _, shp = eng.table["head.w"]
    head_w = eng.blob[o:o + int(np.prod(shp))].cpu().numpy().view(np.int8).reshape(shp)
    want_cam, want_map = class_map_reference(tok8.cpu().numpy(), head_w, idx.cpu().numpy(), eng.class_scale.cpu().numpy())
    same = same and bool(np.array_equal(cam32.cpu().numpy(), want_cam))
    same = same and bool(np.array_equal(maps.cpu().numpy().reshape(want_map.shape).view(np.uint32), want_map.view(np.uint32)))
    if parent is not None:
        pcfg = parent.SWIN_CONFIGS[name]
        peng = parent.swin_engine.SwinEngine(pcfg, weights, scales)
        variants["parent_forward"] = lambda: peng.forward(imgs, nslices=nslices)
        variants["parent_predict"] = lambda: peng.predict(imgs, k=5, nslices=nslices)
        same = same and bool(torch.equal(peng.forward(imgs, nslices=nslices), fwd))
        pi, pv = peng.predict(imgs, k=5, nslices=nslices)
        same = same and bool(torch.equal(pi, pred[0])) and bool(torch.equal(pv.view(torch.int32), pred[1].view(torch.int32)))
    t, rounds = interleaved(variants, reps, warmup=5)
    pairs = [("class_map", "predict"), ("class_map", "forward"), ("class_map_given_headless", "forward")]
    if parent is not None:
        pairs += [("class_map", "parent_predict"), ("forward", "parent_forward"), ("predict", "parent_predict")]
    diff = {f"{a}_minus_{b}": spread(np.asarray(rounds[a]) - np.asarray(rounds[b])) for a, b in pairs}
    print(json.dumps({"what": "class_map vs predict and forward", "model": name, "batch": B, "nslices": nslices, "rounds": reps, "us": t,
                      "differences_us_per_round": diff, "same_integers": same}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--parent", default=None, help="another checkout (built) whose forward and predict are timed in turn with this one's")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    parent = None
    if args.parent:
        parent = load_package(args.parent, "ivit_amd_parent")
        importlib.import_module("ivit_amd_parent.swin_engine")
        assert os.path.dirname(parent._lib.SO_PATH).startswith(os.path.abspath(args.parent)), parent._lib.SO_PATH
    bench_operator(2 * args.reps)
    for nslices in (1, 2):
        bench_model("swin_tiny", "swin_tiny_b1.npz", 256, args.reps, nslices, parent)


if __name__ == "__main__":
    main()
