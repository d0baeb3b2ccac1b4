"""Float weights and calibrated scales -> one model file (include/ivit_modelfile.h, ivit_amd.model_file): the counterpart of the
reference's `TVM_benchmark/convert_model.py` — convert once to integer parameters on disk, then run the integer graph from them.

    python tools/freeze.py --model deit_tiny --golden tests/golden/deit_tiny_b1.npz --out deit_tiny.ivit
    python tools/freeze.py --model swin_tiny --state-dict checkpoint.pth.tar --out swin_tiny.ivit

The model is a name from ivit_amd.CONFIGS / SWIN_CONFIGS with --golden F (the seeded synthetic weights and the scales recorded in a
tests/golden fixture) or --state-dict F (a reference state dict / checkpoint), as in tools/evaluate.py.  Host only: no device and no
library are needed.  Prints one JSON line {"model", "kind", "out", "bytes", "records", "scalars", "input_scale"}.  The file is what
`--model-file` of the other tools, `ivit_amd.load_engine` and the C library's `ivit_model_open` take (examples/classify.c)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ivit_amd as iv  # noqa: E402
from ivit_amd import model_file  # noqa: E402


def load_float_model(model, golden, state_dict):
    """(cfg, float weights, scales) of --model with --golden or --state-dict, as tools/evaluate.py::build_engine reads them"""
    swin = model in iv.SWIN_CONFIGS
    cfg = (iv.SWIN_CONFIGS if swin else iv.CONFIGS)[model]
    if state_dict:
        from ivit_amd.checkpoint import split_state_dict
        weights, scales, _ = split_state_dict(state_dict)
    else:
        g = np.load(golden)
        if str(g["cfg_name"]) != model:
            raise SystemExit(f"{golden} was recorded for {g['cfg_name']}, not {model}")
        scales = {k[len("scale/"):]: np.float32(g[k]) for k in g.files if k.startswith("scale/")}
        weights = (iv.make_swin_weights if swin else iv.make_vit_weights)(cfg, int(g["seed"]))
    return cfg, weights, scales


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", required=True)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--golden")
    src.add_argument("--state-dict")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    cfg, weights, scales = load_float_model(args.model, args.golden, args.state_dict)
    model_file.freeze_to_file(cfg, weights, scales, args.out)
    kind, _, blob, table, scalars, extras = model_file.read(args.out)        # what was written loads
    print(json.dumps({"model": args.model, "kind": kind, "out": args.out, "bytes": os.path.getsize(args.out), "records": len(table) + len(extras),
                      "scalars": len(scalars), "input_scale": scalars["input.s"][1]}))


if __name__ == "__main__":
    main()
