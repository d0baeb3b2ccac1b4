"""Input rules of the scale sweep (tests/golden/scale_sweep.npz), shared by tools/make_scale_sweep_fixture.py, which
feeds these blocks to the reference, and by tests/test_scale_sweep_{cpu,gpu}.py, which rebuild them and compare with the
stored copies.  The blocks cover an operator's input domain instead of sampling it; every draw is seeded."""
import numpy as np

SHIFTMAX_N = (17, 49, 144, 197, 260)
SHIFTMAX_BITS = {17: 16, 49: 8, 144: 8, 197: 16, 260: 16}
MASK_NW, MASK_H, MASK_N = 4, 3, 49
LN_C = (64, 96, 128, 192, 384)
LN_ROWS = 40
QIN_OFFSETS = (0.5, -0.5, 0.49999, 0.0, 0.25)
RQ_C = 64
RQ_ROWS = 48


def csum(a):
    """order-sensitive 64-bit checksum of an integer array (the one of tools/make_golden.py)"""
    a = np.asarray(a).astype(np.int64).reshape(-1)
    idx = np.arange(1, a.size + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return np.uint64(((a.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ idx).sum())


def shiftmax_rows(n):
    """259 rows of length n.  Row r < 256 has maximum r - 128 and holds the largest min(n, r + 1) values at or below it,
    then a seeded random tail of values at or below the maximum, all under a seeded permutation (at n = 260 a row holds
    all 256 values).  Rows 256..258: flat -128, flat 127, one-hot (127 among -128)."""
    rng = np.random.Generator(np.random.PCG64(1000 + n))
    x = np.empty((259, n), np.int8)
    for r in range(256):
        mx = r - 128
        head = np.arange(mx, max(mx - n, -129), -1)
        tail = rng.integers(-128, mx + 1, n - head.size)
        x[r] = np.concatenate([head, tail])[rng.permutation(n)]
    x[256] = -128
    x[257] = 127
    x[258] = -128
    x[258, n // 3] = 127
    return x


def masked_rows():
    """the n = 49 rows repeated over [B_ = nW, H, 49] query rows, and the 0 / -100.0 mask of a shifted 14 x 14 map"""
    base = shiftmax_rows(MASK_N)
    rows = MASK_NW * MASK_H * MASK_N
    x = base[np.arange(rows) % base.shape[0]]
    img = np.zeros((14, 14), np.float32)
    cnt = 0
    for h in (slice(0, -7), slice(-7, -3), slice(-3, None)):
        for w in (slice(0, -7), slice(-7, -3), slice(-3, None)):
            img[h, w] = cnt
            cnt += 1
    mw = img.reshape(2, 7, 2, 7).transpose(0, 2, 1, 3).reshape(4, 49)
    am = mw[:, None, :] - mw[:, :, None]
    mask = np.where(am != 0, np.float32(-100.0), np.float32(0.0)).astype(np.float32)
    return np.ascontiguousarray(x), mask


def gelu_block():
    """256 x 256: row r holds min(v, r - 128) for v = -128..127 — every (row max, Q <= row max) pair once"""
    v = np.arange(-128, 128)
    return np.minimum(v[None, :], (np.arange(256) - 128)[:, None]).astype(np.int8)


def ln_block(C):
    """40 rows: 38 Gaussian rows with amplitudes 2 .. 30 000 (geometric), one zero-variance row, one row alternating
    32767 / -32768; weights with 0.003 and -0.5 among them"""
    rng = np.random.Generator(np.random.PCG64(2000 + C))
    amp = 2.0 * (30000.0 / 2.0) ** (np.arange(LN_ROWS - 2) / (LN_ROWS - 3))
    x = np.clip(np.rint(rng.standard_normal((LN_ROWS - 2, C)) * amp[:, None]), -32768, 32767).astype(np.int16)
    flat = np.full((1, C), 7, np.int16)
    alt = np.where(np.arange(C) % 2 == 0, 32767, -32768).astype(np.int16)[None]
    x = np.concatenate([x, flat, alt])
    w = (1.0 + rng.standard_normal(C) * 0.4).astype(np.float32)
    w[0] = 0.003
    w[1] = -0.5
    b = (rng.standard_normal(C) * 0.5).astype(np.float32)
    return x, w, b


LN_TOKEN_C = (64, 96, 128, 192)
LN_TOKENS = 49


def ln_token_block(C):
    """two images of 49 tokens (rows of ln_block(C), repeated): both of torch's strided-sum orders occur — groups of 32
    tokens and the 17 left over — and a block of rows spans the image boundary"""
    x, w, b = ln_block(C)
    return np.ascontiguousarray(x[np.arange(2 * LN_TOKENS) % LN_ROWS]), w, b


def qin_grid():
    """(k + offset) for k = -140..140 and the five offsets: ties, near-ties and saturation at every scale"""
    k = np.arange(-140, 141, dtype=np.float32)
    return (k[:, None] + np.asarray(QIN_OFFSETS, np.float32)[None, :]).astype(np.float32).reshape(-1)


def qin_values(scale):
    return (qin_grid() * np.float32(scale)).astype(np.float32)


def _neighbours(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(np.inf))]


def rq_ratios(zmax):
    """64 per-channel multipliers s_pre / s_out (float32): log-uniform over 2^-30 .. 2^12, powers of two (exact .5 ties),
    both float32 neighbours of 512, 1024, 2048 and 2^31 / zmax, 512 / 1024 / 2048 themselves and 600; every seventh
    negative (an I-LayerNorm channel with a negative weight)"""
    rng = np.random.Generator(np.random.PCG64(3000))
    r = [np.float32(2.0 ** -k) for k in (1, 2, 3, 5, 8, 12, 20, 30)] + [np.float32(1), np.float32(4)]
    for b in (512.0, 1024.0, 2048.0, 2.0 ** 31 / zmax):
        r += _neighbours(b)
    r += [np.float32(512), np.float32(1024), np.float32(2048), np.float32(600), np.float32(4096)]
    r += list((2.0 ** rng.uniform(-30, 12, RQ_C - len(r))).astype(np.float32))
    r = np.asarray(r, np.float32)
    assert r.size == RQ_C
    r[6::7] *= np.float32(-1)
    return r


def rq_block(zmax, ratios):
    """[48, 64] integers.  Rows 0..15: in the channels whose multiplier is 2^-k, odd multiples of 2^(k-1) (exact .5 ties of
    either sign) where they fit, seeded draws elsewhere.  Rows 16..27 and 28..39: the integers whose product with the
    channel's multiplier is spread over 1.3 times the 8-bit and the 16-bit output range (where |z| <= zmax allows), so each
    width saturates on part of a channel only.  Rows 40..45: seeded draws of growing amplitude; the last two rows +-zmax."""
    rng = np.random.Generator(np.random.PCG64(3100 + int(zmax) % 977))
    amp = 2.0 * (zmax / 2.0) ** (np.arange(RQ_ROWS) / (RQ_ROWS - 1))
    z = np.rint(rng.uniform(-1, 1, (RQ_ROWS, RQ_C)) * amp[:, None]).astype(np.int64)
    a = ratios.astype(np.float64)
    for c, v in enumerate(np.abs(a)):
        k = -np.log2(v)
        if k >= 1 and k == np.floor(k):
            for r in range(16):
                t = (2 * r + 1) * 2 ** (int(k) - 1) * (-1 if r % 2 else 1)
                if abs(t) <= zmax:
                    z[r, c] = t
    for r0, lim in ((16, 128.0), (28, 32768.0)):
        target = rng.uniform(-1.3 * lim, 1.3 * lim, (12, RQ_C))
        t = np.rint(target / a[None, :])
        ok = np.abs(t) <= zmax
        z[r0:r0 + 12][ok] = t[ok].astype(np.int64)
    z[-2] = zmax
    z[-1] = -zmax
    return np.clip(z, -zmax - 1, zmax).astype(np.int32)


RQ_CASES = [(zname, bits, ident) for zname in ("z16", "z21") for bits in (8, 16) for ident in (0, 1, 2)]
RQ_ZMAX = {"z16": 32767, "z21": 1500000}
RQ_ID_RATIO = {1: np.float32(0.37), 2: np.float32(700.0)}
RQ_S_OUT = np.float32(2.0 ** -4)


def rq_identity():
    """[48, 64] identity integers of the 16-bit range, the row amplitude growing from 1 to 32767"""
    rng = np.random.Generator(np.random.PCG64(3200))
    amp = 32767.0 ** (np.arange(RQ_ROWS) / (RQ_ROWS - 1))
    return np.rint(rng.uniform(-1, 1, (RQ_ROWS, RQ_C)) * amp[:, None]).astype(np.int32)
