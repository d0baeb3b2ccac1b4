"""Operands at which the reference's dyadic requant and a single fused rounding give different integers.

The reference (quant_utils.py:229-230) computes  two(z) = RNE(fl64(z * m) * 2^-e): the product is rounded to 53 bits first.  The
one-FMA epilogue computes  one(z) = RNE(z * m * 2^-e)  of the exact product.  They differ only where |z * m| >= 2^53 and the exact
product lies within half an ulp of fl64 of a tie, that is  z * m = 2^(e-1) + d  (mod 2^e)  for a small d != 0.  For an odd m that
is one residue class of z per d, found with the modular inverse of m; the candidates are then checked with exact integer
arithmetic against numpy float64.  Everything here is deterministic: a seeded generator and a bounded number of tries.

K = 1536 (fc2 of the width-384 Mlp): |z| <= 128 * 127 * 1536, the accumulator's own range, so that the bias the GPU tests use to
steer one element onto z stays as small as the accumulator.  K = 384: |z| <= 128 * 127 * 384 < 2^23 together with
|z * m| >= 2^53 leaves m > 1.44e9 and a window of about 10^6 values of z per sign; the bounded search below finds its triples
inside that range, so no bias term has to carry z there either.  The 8-bit range needs e >= 47 (at e = 46 and |z * m| >= 2^53
every result is +-128 or beyond and the clamp hides the difference); search_8bit looks there, with a larger bound.
"""
import numpy as np

E16 = 40                                         # 2^-e of the 16-bit triples: results z * m * 2^-40 with m in [2^30, 2^31)
ZMAX = {1536: 128 * 127 * 1536, 384: 128 * 127 * 384}
SEEDS = {1536: 15360, 384: 3840}
PER_SIGN = 4
MAX_TRIES = 1 << 23                              # multipliers drawn at most, per search
_BLOCK = 1 << 18


def rne_shift(p, e):
    """RNE(p / 2^e) of a Python integer, exactly"""
    q, r = divmod(p, 1 << e)
    half = 1 << (e - 1)
    return q + 1 if r > half or (r == half and (q & 1)) else q


def one_rounding(z, m, e):
    return rne_shift(int(z) * int(m), e)


def two_roundings(z, m, e):
    """the reference's order: the product in float64, scaled by the power of two (exact), rounded to nearest even"""
    return int(np.rint((np.float64(int(z)) * np.float64(int(m))) * np.float64(2.0 ** -e)))


def differing(m, e, zmax, lim=32767, dmax=4):
    """Every z in [-zmax, zmax] with one_rounding != two_roundings and both within +-lim, for any integer m > 0 (zmax * m < 2^56:
    half an ulp of the product is at most dmax).  Exact: the residue classes of z * m = 2^(e-1) + d (mod 2^e), |d| <= dmax."""
    assert m > 0 and zmax * m < 1 << 56
    t = (m & -m).bit_length() - 1
    mod = 1 << (e - t)
    inv = pow(m >> t, -1, mod)
    out = []
    for d in range(-dmax, dmax + 1):
        target = (1 << (e - 1)) + d
        if d == 0 or target % (1 << t):
            continue
        z = (inv * (target >> t)) % mod
        z -= ((z + zmax) // mod) * mod           # the smallest member of the class >= -zmax
        while z <= zmax:
            a, b = one_rounding(z, m, e), two_roundings(z, m, e)
            if a != b and max(abs(a), abs(b)) <= lim:
                out.append(z)
            z += mod
    return sorted(out)


def _inverse_mod_2_64(m):
    """modular inverse of odd uint64 values mod 2^64 (Newton: m is its own inverse mod 8, each step doubles the bits)"""
    x = m.copy()
    for _ in range(5):
        x = x * (np.uint64(2) - m * x)
    return x


def search(zmax, seed, e=E16, lim=32767, per_sign=PER_SIGN, max_tries=MAX_TRIES):
    """(z, m, e, one, two) with m odd in [2^30, 2^31), |z| <= zmax, |z * m| >= 2^53, both results within +-lim and different:
    the first per_sign with z > 0 and the first per_sign with z < 0 in the order the seeded draws give them.  Fewer (or none) if
    max_tries multipliers do not yield them."""
    rng = np.random.default_rng(seed)
    found = {1: [], -1: []}
    mask = np.uint64((1 << e) - 1)
    with np.errstate(over="ignore"):
        for _ in range(max_tries // _BLOCK):
            m = rng.integers(1 << 29, 1 << 30, _BLOCK, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
            inv = _inverse_mod_2_64(m)
            for d in (1, -1, 2, -2, 3, -3):
                zr = ((inv * np.uint64((1 << (e - 1)) + d)) & mask).astype(np.int64)
                z = np.where(zr >= 1 << (e - 1), zr - (1 << e), zr)
                for i in np.nonzero(np.abs(z) <= zmax)[0]:
                    zi, mi = int(z[i]), int(m[i])
                    if abs(zi) * mi < 1 << 53:
                        continue
                    assert (zi * mi) % (1 << e) == (1 << (e - 1)) + d
                    a, b = one_rounding(zi, mi, e), two_roundings(zi, mi, e)
                    sign = 1 if zi > 0 else -1
                    if a != b and max(abs(a), abs(b)) <= lim and len(found[sign]) < per_sign:
                        found[sign].append((zi, mi, e, a, b))
            if all(len(v) >= per_sign for v in found.values()):
                break
    return found[1] + found[-1]


def search_16bit(K):
    return search(ZMAX[K], SEEDS[K])


def search_8bit(K=1536, max_tries=1 << 25):
    """the same in the 8-bit range (results within +-127): one triple of each sign at e = 47, 48 and 49.  About one multiplier in
    10^7 has one, so the bound is 2^25 draws per e (seconds; tools/make_requant_two_roundings_fixture.py runs it, the tests read
    the fixture).  |z| of these is above 10^7: in a K = 384 layer the bias carries it."""
    out = []
    for e in (47, 48, 49):
        out += search(ZMAX[K], 8000 + e, e=e, lim=127, per_sign=1, max_tries=max_tries)
    return out
