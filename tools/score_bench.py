"""Timing of the score launch on the device (profiles/README.md, "Score"): ivit_logits_score (rank and nll of every label) beside
ivit_logits_topk(k = 5) on the same 256 x 1000 logits, and at batch 1.  The method is tools/topk_bench.py's: medians of HIP-event
times with quartiles and extremes, the two launches alternating inside one loop, each also timed as a train of 20 launches between
one pair of events.  Prints one JSON line per shape.   python tools/score_bench.py [--reps 200]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ivit_amd import _lib  # noqa: E402
from ivit_amd.predict import score_reference  # noqa: E402
from topk_bench import interleaved  # noqa: E402

_P = ctypes.c_void_p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    H = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(0)
    for B in (256, 1):
        acc = rng.integers(-2 ** 20, 2 ** 20, size=(B, 1000), dtype=np.int64).astype(np.int32)
        sc = rng.uniform(1e-6, 1e-5, size=1000).astype(np.float32)
        lab = rng.integers(0, 1000, size=B).astype(np.int64)
        logits, scale, labels = (torch.from_numpy(a).cuda() for a in (acc, sc, lab))
        idx = torch.empty(B, 5, dtype=torch.int32, device="cuda")
        val = torch.empty(B, 5, dtype=torch.float32, device="cuda")
        rank = torch.empty(B, dtype=torch.int32, device="cuda")
        nll = torch.empty(B, dtype=torch.float64, device="cuda")
        topk = (_P(logits.data_ptr()), _P(scale.data_ptr()), B, 1000, 5, _P(idx.data_ptr()), _P(val.data_ptr()))
        score = (_P(logits.data_ptr()), _P(scale.data_ptr()), _P(labels.data_ptr()), B, 1000, _P(rank.data_ptr()), _P(nll.data_ptr()))
        variants = {"ivit_logits_topk_k5": lambda: H.call("ivit_logits_topk", *topk),
                    "ivit_logits_score": lambda: H.call("ivit_logits_score", *score),
                    "ivit_logits_score_rank_only": lambda: H.call("ivit_logits_score", *score[:-1], None)}
        H.call("ivit_logits_score", *score)
        torch.cuda.synchronize()
        want_rank, want_nll = score_reference(acc, sc, lab)
        same = bool(np.array_equal(rank.cpu().numpy(), want_rank)) and bool(np.allclose(nll.cpu().numpy(), want_nll, rtol=1e-12, atol=1e-9))
        print(json.dumps({"what": "score launch", "shape": [B, 1000], "single_call_us": interleaved(variants, args.reps)[0],
                          "train_of_20_us_per_call": interleaved(variants, max(20, args.reps // 4), train=20)[0],
                          "equal_to_reference": same}), flush=True)


if __name__ == "__main__":
    main()
