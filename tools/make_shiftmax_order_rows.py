"""Searches 144-wide int8 Shiftmax rows (8-bit output, scale 0.0523) whose probabilities depend on the ORDER of the exp_int
row sum: torch's order (the oracle's torch_sum) and a plain sequential sum give different F = floor(2^31/S)
and hence different P.  Random rows almost never do (F ~ 80: a 1-2 ulp change of S rarely crosses an integer), so the
fixture tests/golden/shiftmax144_order_rows.npz keeps the few found, for the window-12 tests.  CPU only, ~1 min.

    python tools/make_shiftmax_order_rows.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as orc  # noqa: E402
from shiftmax144 import exps, probs, sum_a7, sum_seq  # noqa: E402

SCALE = np.float32(0.0523)


def main(want=8):
    rng = np.random.default_rng(0)
    found = []
    for _ in range(600):
        n = 20000
        top = rng.integers(60, 128, (n, 1))
        k = rng.integers(1, 40, (n, 1))
        a = np.clip(top - np.minimum(rng.geometric(1.0 / k, (n, 144)) - 1, 255), -128, 127).astype(np.int8)
        e = exps(a, SCALE)
        pa, ps = probs(e, sum_a7(e)), probs(e, sum_seq(e))
        found += [a[i] for i in np.nonzero((pa != ps).any(axis=1))[0]]
        if len(found) >= want:
            break
    rows = np.array(found[:want], np.int8)
    assert np.array_equal(orc.shiftmax(rows, SCALE, 8).astype(np.int32), probs(exps(rows, SCALE), sum_a7(exps(rows, SCALE))))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "shiftmax144_order_rows.npz"), rows=rows, scale=SCALE)
    print("rows", rows.shape)


if __name__ == "__main__":
    main()
