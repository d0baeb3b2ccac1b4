"""Generate tests/golden/runner_refusals.json: the status and the full text of ivit_last_error that a library gives for every
refused call of tests/runner_refusal_cases.py — every eager runner entry of micro_vit_b2 and micro_swin_b2 at batch 2, each call
breaking exactly one rule.  tests/test_runner_refusals_gpu.py holds the library of the tree to this record.

Run it against the library whose answers are to be pinned — IVIT_LIB names it; the binding of this tree loads it as long as the
C-ABI is the same — on a machine with a HIP device:

    IVIT_LIB=/path/to/the/pinned/libivit_hip.so python tools/make_runner_refusals_fixture.py

A refusal whose text a change rewrites on purpose is then edited in the fixture by hand, and the test's docstring says which.
The case "m null" has no text: a null model has no handle to leave one in.  Every call is checked to have left the entry's
arrays as they were; the unmodified call of each entry must then succeed.
"""
import json
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import runner_refusal_cases as rc  # noqa: E402
from ivit_amd import _lib  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "runner_refusals.json")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    golden = lambda name: np.load(os.path.join(GOLDEN, name), allow_pickle=False)
    scales = lambda g: {k[len("scale/"):]: np.float32(g[k]) for k in g.files if k.startswith("scale/")}
    record = {}
    for fname in rc.MODELS:
        g, cfg, eng, imgs = rc.engine(fname, golden, scales)
        record[fname] = {}
        for key, (symbol, params) in rc.entries(cfg, eng, imgs).items():
            mem, _ = rc.arenas(params)
            before = {n: t.clone() for n, t in mem.items()}
            rows = []
            for name, change in rc.refusals(params, eng.MAX_SLICES):
                st, text = rc.run(eng, symbol, params, mem, change)
                assert st != _lib.IVIT_OK, (fname, key, name, "was accepted")
                rows.append({"case": name, "status": st, "error": None if name == "m null" else text})
            torch.cuda.synchronize()
            assert all(torch.equal(mem[n], before[n]) for n in mem), (fname, key, "a refused call wrote")
            if "workspace" in mem:
                eng._workspace_init(mem["workspace"], rc.B, 1)
            st, text = rc.run(eng, symbol, params, mem)
            torch.cuda.synchronize()
            assert st == _lib.IVIT_OK, (fname, key, text)
            lg = rc.good_logits(params, mem, cfg.num_classes)
            assert lg is None or np.array_equal(lg, g["logits_int"]), (fname, key)
            record[fname][key] = rows
            print(fname, key, len(rows), "refusals")
    with open(OUT, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes, library", _lib.SO_PATH)


if __name__ == "__main__":
    main()
