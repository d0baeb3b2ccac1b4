"""Generate tests/golden/requant_two_roundings.npz: what the reference's own dyadic requant (fixedpoint_mul.forward,
quant_utils.py:178-253) gives at the operands of tests/two_roundings.py, where rounding the product z * m to float64 before the
shift changes the integer (tests/test_requant_two_roundings_cpu.py, tests/test_requant_two_roundings_gpu.py).

Runs ONLY in the build container (needs the reference tree + torch CPU), like tools/make_scale_sweep_fixture.py.  The fixture is
data: per K the triples (z, m, e), the reference's result `two` and, beside it, the exact single rounding `one`.

    python tools/make_requant_two_roundings_fixture.py
"""
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, _HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_harness as rh  # noqa: E402
import two_roundings as tr  # noqa: E402
from make_scale_sweep_fixture import save_deterministic  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "requant_two_roundings.npz")


def reference_requant(fixedpoint_mul, z, m, e, bits):
    """fixedpoint_mul on pre_act = z * s with s = m * 2^-e and an output scale of 1: batch_frexp of s / 1 gives back (m, e) exactly
    (m < 2^31 is its own 31-bit mantissa).  Everything is handed over in float64, so that the module's round(pre_act / s) is z itself."""
    s = torch.tensor([float(m) * 2.0 ** -e], dtype=torch.float64)
    pre = torch.tensor([[float(z)]], dtype=torch.float64) * s
    assert torch.round(pre / s).item() == float(z)
    out = fixedpoint_mul.apply(pre, s, bits, "symmetric", torch.tensor(1.0))
    return int(out.item())


def main():
    rh.load_reference()
    from models.quantization_utils.quant_utils import batch_frexp, fixedpoint_mul
    d = {}
    for K in sorted(tr.ZMAX):
        rows = []
        for z, m, e, one, two in tr.search_16bit(K):
            mm, ee = batch_frexp(torch.tensor([float(m) * 2.0 ** -e], dtype=torch.float64))
            assert int(mm.item()) == m and int(ee.item()) == e
            ref = reference_requant(fixedpoint_mul, z, m, e, 16)
            assert ref == two and ref != one, (z, m, e, ref, one, two)
            rows.append((z, m, e, ref, one))
        assert sum(r[0] > 0 for r in rows) >= tr.PER_SIGN and sum(r[0] < 0 for r in rows) >= tr.PER_SIGN, K
        d[f"k{K}"] = np.asarray(rows, np.int64)          # columns: z, m, e, two (the reference), one
        print(f"K = {K}:")
        for r in rows:
            print("   z %9d  m %10d  e %d  reference %6d  one rounding %6d" % r)
    found8 = tr.search_8bit()
    rows = [(z, m, e, reference_requant(fixedpoint_mul, z, m, e, 8), one) for z, m, e, one, two in found8]
    assert all(r[3] == f[4] != r[4] for r, f in zip(rows, found8))
    d["bits8"] = np.asarray(rows, np.int64).reshape(-1, 5)
    print(f"8-bit range: {len(rows)} triples", rows)
    save_deterministic(OUT, d)
    print("requant_two_roundings.npz bytes", os.path.getsize(OUT))


if __name__ == "__main__":
    main()
