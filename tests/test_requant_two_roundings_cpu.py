"""The dyadic requant where its two roundings matter: operands (z, m, e) at which RNE(fl64(z * m) * 2^-e), the reference's order
(quant_utils.py:229-230), and RNE(z * m * 2^-e), one rounding of the exact product, are different integers
(tests/two_roundings.py finds them; tests/golden/requant_two_roundings.npz holds what the reference itself returned for each,
recorded by tools/make_requant_two_roundings_fixture.py, and the single rounding beside it).  The CPU oracle and the CPU twin of the
C-ABI must give the reference's integer; tests/test_requant_two_roundings_gpu.py asks the same of every HIP epilogue."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden

from oracle import oracle as orc
import two_roundings as tr
from abi_cases import load_twin

_P = ctypes.c_void_p
KS = (1536, 384)


@pytest.fixture(scope="module")
def g():
    z = load_golden("requant_two_roundings.npz")
    return {k: z[k] for k in z.files}


def odv(m, e):
    d = (orc.Dyadic * 1)()
    d[0].m, d[0].r = float(m), 2.0 ** -e
    return d


def test_fixture_is_what_the_search_finds(g):
    """the helper is deterministic and bounded: it reproduces the recorded triples, at least four of each sign per K, inside the
    accumulator's own range, with products past 2^53 and results inside the 16-bit range"""
    for K in KS:
        rows = g[f"k{K}"]
        assert np.array_equal(rows[:, :3], np.asarray([r[:3] for r in tr.search_16bit(K)], np.int64)), K
        assert (rows[:, 0] > 0).sum() >= 4 and (rows[:, 0] < 0).sum() >= 4
        for z, m, e, two, one in rows.tolist():
            assert abs(z) <= tr.ZMAX[K] and abs(z) * m >= 1 << 53 and m & 1 and 1 << 30 <= m < 1 << 31 and e == tr.E16
            assert max(abs(one), abs(two)) <= 32767
            assert z in tr.differing(m, e, tr.ZMAX[K])
    # the 8-bit range: recorded by the tool's longer search (not repeated here); each is a true member of its residue class
    b8 = g["bits8"]
    print("8-bit-range triples recorded:", b8.tolist())
    assert (b8[:, 0] > 0).sum() >= 1 and (b8[:, 0] < 0).sum() >= 1
    for z, m, e, two, one in b8.tolist():
        assert e >= 47 and abs(z) <= tr.ZMAX[1536] and max(abs(one), abs(two)) <= 127 and z in tr.differing(m, e, tr.ZMAX[1536], lim=127)


def test_the_two_orders_differ_at_every_triple(g):
    for K in KS + ("bits8",):
        for z, m, e, two, one in g[K if K == "bits8" else f"k{K}"].tolist():
            assert abs(two - one) == 1, (z, m, e)
            assert tr.one_rounding(z, m, e) == one and tr.two_roundings(z, m, e) == two, (z, m, e)


def test_oracle_and_twin_give_the_reference(g):
    twin = load_twin()
    for K in KS + ("bits8",):
        rows = g[K if K == "bits8" else f"k{K}"]
        bits = 8 if K == "bits8" else 16
        for z, m, e, two, one in rows.tolist():
            zz = np.array([[z]], np.int32)
            assert orc.requant(zz, odv(m, e), bits)[0, 0] == two, (z, m, e)
            assert orc.requant(zz.astype(np.float32), odv(m, e), bits)[0, 0] == two, (z, m, e)      # |z| < 2^24: exact in fp32
            fd = np.array([[float(m), 2.0 ** -e]], np.float64)
            out = np.zeros((1, 1), np.int8 if bits == 8 else np.int16)
            for name, arr in (("requant_i32", zz), ("requant_f32", zz.astype(np.float32))):
                assert getattr(twin, "ivit_cpu_" + name)(None, arr.ctypes.data_as(_P), fd.ctypes.data_as(_P), 1, None, None, bits,
                                                         out.ctypes.data_as(_P), 1, 1) == 0
                assert int(out[0, 0]) == two, (name, z, m, e)
