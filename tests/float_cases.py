"""The case lists of the two float-accumulating operators (include/ivit_logreg.h, include/ivit_gauss.h), shared by their GPU suites
(tests/test_logreg_gpu.py, tests/test_gauss_gpu.py, tests/test_float_contract_gpu.py), the CPU suite that checks the lists themselves
(tests/test_float_cases_cpu.py) and the two error-measuring tools (tools/logreg_bench.py --errors, tools/gauss_bench.py --errors), so
that a tool measures exactly the cases a test bounds.  numpy only: nothing here needs a device, torch or the package.

  logreg_case / gauss_arrays   the suites' data generators (one normal distribution per array)
  WIDTHS, *_WIDTH_CASES        every width the launchers dispatch on: `switch (dim / 64)` and `switch ((dim / 32 + 3) / 4)`
  LOGREG_FLUSH_CASES           both sides of LOGREG_FLUSH_ROWS, with logreg_layout, the launcher's part arithmetic restated
  onehot_*                     models whose table rows hold ONE nonzero weight each: every z and s is a single exact product, so
                               ivit_gauss_score's four outputs are known bit for bit (onehot_gauss_expected)
  launched_instantiations      which template instantiations a list of cases starts"""
import functools

import numpy as np

# ---------------------------------------------------------------- the suites' generators
def logreg_case(N, C, dim, seed=0):
    """x, labels, W, b, x_scale with logits of about unit size"""
    rng = np.random.default_rng([N, C, dim, seed])
    return (rng.integers(-128, 128, size=(N, dim)).astype(np.int8), rng.integers(C, size=N).astype(np.int32),
            (rng.normal(size=(C, dim)) * 0.3 / np.sqrt(dim)).astype(np.float32), rng.normal(size=C).astype(np.float32), 0.05)


def gauss_arrays(N, dim, R, C, seed=0):
    """x, Wh, t, Wc, bc of a model whose q and scores are of unit-to-R size"""
    rng = np.random.default_rng([N, dim, R, C, seed])
    x = rng.integers(-128, 128, size=(N, dim)).astype(np.int8)
    Wh, t = (rng.normal(size=(R, dim)) / (74 * np.sqrt(dim))).astype(np.float32), rng.normal(size=R).astype(np.float32)
    Wc, bc = (4 * rng.normal(size=(C, dim)) / (74 * np.sqrt(dim))).astype(np.float32), rng.normal(size=C).astype(np.float32)
    return x, Wh, t, Wc, bc


# ---------------------------------------------------------------- A: every dispatched width
MIN_DIM, MAX_DIM = 64, 1024                 # LOGREG_ / GAUSS_MIN_DIM, _MAX_DIM of csrc/ivit_logreg.h, csrc/ivit_gauss.h
WIDTHS = list(range(MIN_DIM, MAX_DIM + 1, 64))
# N = 129: one full 128-row block and a ragged 32-row step of one row; C = 33: a full class tile and a one-class tile.
# (N, C, dim, splits, seed).  splits: one part, the library's (one part at N < 512), 9 (more than the five 32-row steps: five parts
# of one step each), 3
LOGREG_WIDTH_CASES = [(129, 33, dim, (1, 0, 9, 3)[i % 4], 0) for i, dim in enumerate(WIDTHS)]
# (N, dim, R, C, splits, seed).  R = 32 at every width (three tiles), R = dim at the two widths of the workload's backbones;
# splits: one part, the library's (a part per tile at two row blocks), 5 (more than the three tiles), 2; 16 (more than the 14 tiles
# of R = 384) and 1 at R = dim
GAUSS_WIDTH_CASES = [(129, dim, 32, 33, (1, 0, 5, 2)[i % 4], 0) for i, dim in enumerate(WIDTHS)] + [(129, 384, 384, 33, 16, 0), (129, 768, 768, 33, 1, 0)]


def launched_instantiations(dims):
    """the template arguments the launchers of csrc/ivit_hip.hip pick for these widths: (KS of logreg_rows_kernel<KS> and
    gauss_score_kernel<KS>: `switch (dim / 64)`; NT of logreg_grad_kernel<NT>: `switch ((dim / 32 + 3) / 4)`)"""
    return sorted({d // 64 for d in dims}), sorted({(d // 32 + 3) // 4 for d in dims})


def compiled_instantiations():
    """what the two `switch` statements hold a case label for: every supported width"""
    return launched_instantiations(range(MIN_DIM, MAX_DIM + 1, 64))


# ---------------------------------------------------------------- B: both sides of LOGREG_FLUSH_ROWS
LOGREG_TILE, LOGREG_PIECES, LOGREG_ROW_BYTES, LOGREG_FLUSH_ROWS = 32, 3, 16, 65536      # csrc/ivit_logreg.h
# (N, C, dim, splits, seed): one part of exactly LOGREG_FLUSH_ROWS rows; one row more, one part asked for: two parts of 32800 and
# 32737 rows; the same with the library's choice of parts.  The seeds: the first whose smallest margin between a label's logit and
# the largest other one is well above 1e-5 max|z| (tests/test_float_cases_cpu.py)
LOGREG_FLUSH_CASES = [(65536, 33, 64, 1, 2), (65537, 33, 64, 1, 1), (65537, 33, 64, 0, 1)]


def logreg_layout(N, dim, C, splits, cus):
    """logreg_shape_bad of csrc/ivit_hip.hip restated -> dict(tiles, parts, per, bytes).  cus > 0: the parts of a launch on that many
    CUs; cus == 0: the size query, which states the most parts any device is given"""
    tiles = (C + LOGREG_TILE - 1) // LOGREG_TILE
    want = splits if splits > 0 else max(1, min((2 * min(cus if cus > 0 else 1024, 1024) + tiles - 1) // tiles, N // 256))
    s = max(want, (N + LOGREG_FLUSH_ROWS - 1) // LOGREG_FLUSH_ROWS)
    per = ((N + s - 1) // s + LOGREG_TILE - 1) // LOGREG_TILE * LOGREG_TILE
    parts = (N + per - 1) // per if cus > 0 or splits > 0 else s
    cpad = tiles * LOGREG_TILE
    nbytes = cpad * dim * 2 * LOGREG_PIECES + N * LOGREG_ROW_BYTES + parts * cpad * dim * 4 + parts * cpad * 4
    return dict(tiles=tiles, parts=parts, per=per, bytes=nbytes)


# ---------------------------------------------------------------- C: one-hot models
ONEHOT_N, ONEHOT_C = 129, 70
ONEHOT_MINUS_INF = (1, 40)                  # classes at -inf: one in each of the first two class tiles
ONEHOT_X_SCALE = 2.0 ** -4                  # the logistic probe's x_scale on these models: a power of two, so every logit stays exact
# (dim, R, splits): R = 32 at every width, R = 96 at three
ONEHOT_GAUSS_CASES = [(dim, 32, (0, 1, 5, 2)[i % 4]) for i, dim in enumerate(WIDTHS)] + [(192, 96, 1), (384, 96, 0), (768, 96, 7)]
ONEHOT_LOGREG_CASES = [(dim, (0, 1, 9, 3)[i % 4]) for i, dim in enumerate(WIDTHS)]
_POWERS = np.array([1, -1, 2, -2, 4, -4, 8, -8, 16, -16, 32, -32, 64, -64, -128], np.int8)


def onehot_columns(dim, R, C=ONEHOT_C):
    """-> (rows of Wh, their columns) of the R / 32 whitening weights (one table row per tile), the columns of the C class weights
    (class k in row k of Wc).  A stride of 37
    features (odd, prime to every dim / 64): consecutive classes fall into different 32-feature pair-steps and alternate between
    the 16-feature halves, any 64 consecutive classes hit every column position of a 64-feature step, and 70 classes reach every
    step of every width"""
    tiles = np.arange(R // 32)
    return 32 * tiles + (5 * tiles + 3) % 32, (53 * tiles + 29 + dim // 64) % dim, (37 * np.arange(C) + 3 * (dim // 64)) % dim


def _full_mantissa_weights(rng, n):
    """n float32 with all 24 significant bits in use (mantissa bits 0, 8 and 16 set: all three bf16 pieces of logreg_split3 are
    nonzero), a random sign, and exponents that step through 2^-30 .. 2^30 by 13 (mod 61): any 32 consecutive ones span the range"""
    mant = rng.integers(0, 1 << 23, size=n, dtype=np.int64) | 1 | (1 << 8) | (1 << 16)
    expo = -30 + (13 * np.arange(n) + 7) % 61
    bits = (rng.integers(0, 2, size=n, dtype=np.int64) << 31) | ((expo + 127).astype(np.int64) << 23) | mant
    return bits.astype(np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def onehot_case(dim, R, N=ONEHOT_N, C=ONEHOT_C):
    """-> x int8 [N, dim], Wh [R, dim], t [R] = 0, Wc [C, dim], bc [C] (0, or -inf on ONEHOT_MINUS_INF): one nonzero weight per
    class row and per whitening tile; x holds a power of two (+-1 .. +-64, -128) wherever a weight is nonzero and arbitrary int8
    elsewhere.  Built once per shape and left unchanged"""
    rng = np.random.default_rng([dim, R, N, C, 2024])
    wrows, wcols, ccols = onehot_columns(dim, R, C)
    Wh, Wc = np.zeros((R, dim), np.float32), np.zeros((C, dim), np.float32)
    Wh[wrows, wcols] = _full_mantissa_weights(rng, len(wrows))
    Wc[np.arange(C), ccols] = _full_mantissa_weights(rng, C)
    bc = np.zeros(C, np.float32)
    bc[list(ONEHOT_MINUS_INF)] = -np.inf
    x = rng.integers(-128, 128, size=(N, dim)).astype(np.int8)
    for col in np.union1d(wcols, ccols):
        x[:, col] = _POWERS[rng.integers(0, len(_POWERS), size=N)]
    for a in (x, Wh, Wc, bc):
        a.setflags(write=False)
    return x, Wh, np.zeros(R, np.float32), Wc, bc


def onehot_gauss_expected(x, Wh, t, Wc, bc):
    """(dist, cls, q, best) as include/ivit_gauss.h's documented order gives them on a one-hot model, in float32 arithmetic: every z
    and s is one exact product (a float32 times a power of two), q = the float32 sum in ascending tile order of float32(z_tile^2),
    best = max_c s with the smallest index on equal values, dist = float32(q - best)"""
    assert not t.any() and all(np.count_nonzero(Wh[i:i + 32]) == 1 for i in range(0, len(Wh), 32)) and (np.count_nonzero(Wc, axis=1) == 1).all()
    xf = x.astype(np.float32)
    q = np.zeros(len(x), np.float32)
    for i in range(0, len(Wh), 32):
        row, col = (int(v[0]) for v in np.nonzero(Wh[i:i + 32]))
        z = Wh[i + row, col] * xf[:, col]                # float32 x float32: exact here, asserted against float64 by the CPU suite
        q = q + z * z                                    # one rounding for the square, one for the sum
    s = Wc[np.arange(len(Wc)), np.argmax(Wc != 0, axis=1)][None, :] * xf[:, np.argmax(Wc != 0, axis=1)] + bc[None, :]
    cls = s.argmax(axis=1).astype(np.int32)
    best = s[np.arange(len(x)), cls]
    return q - best, cls, q, best


@functools.lru_cache(maxsize=None)
def onehot_logreg_case(dim):
    """x, labels, W, b, x_scale for ivit_logreg_loss_grad on the one-hot class table of onehot_case(dim, 32): b = 0 (finite: the
    probe has no empty class), x_scale a power of two, so every logit is one exact product; half of the labels are the row's largest
    logit, the others arbitrary"""
    x, _, _, Wc, _ = onehot_case(dim, 32)
    rng = np.random.default_rng([dim, 77])
    z = x.astype(np.float64) @ Wc.astype(np.float64).T
    lab = np.where(rng.integers(0, 2, size=len(x)) == 1, z.argmax(axis=1), rng.integers(0, len(Wc), size=len(x))).astype(np.int32)
    lab.setflags(write=False)
    return x, lab, Wc, np.zeros(len(Wc), np.float32), ONEHOT_X_SCALE


# ---------------------------------------------------------------- D: the arena harness
LOGREG_CONTRACT_CASES = [(129, 33, 192, 0), (300, 70, 384, 3)]              # (N, C, dim, splits)
GAUSS_CONTRACT_CASES = [(129, 192, 96, 33, 3), (300, 384, 32, 70, 0)]       # (N, dim, R, C, splits)
CONTRACT_TILE_ROWS = 128    # the tallest tile of these kernels: 128 feature rows of a workgroup (32 table rows for the [C, dim] floats)
