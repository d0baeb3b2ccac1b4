"""The case lists of tests/float_cases.py without a GPU: they reach every template instantiation the launchers dispatch on (read from
csrc/ivit_hip.hip), their seeds leave the class decisions to the float64 reference alone, the restated part arithmetic of the logistic
probe on both sides of LOGREG_FLUSH_ROWS, and the one-hot expectation against the float64 statement."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import float_cases as F
from ivit_amd.predict import gauss_score_reference, logreg_reference

CSRC = os.path.join(ROOT, "i-vit_amd", "csrc")


def _dispatch_tables():
    """[(kernel, switch expression, case labels)] of the LOGREG_CASE / GAUSS_CASE switches of csrc/ivit_hip.hip"""
    src = open(os.path.join(CSRC, "ivit_hip.hip")).read()
    found = re.findall(r"switch \(([^\n]*)\) \{[^\n]*\n#define ((?:LOGREG|GAUSS)_CASE)\((\w+)\) case \3: (\w+)<\3>(.*?)#undef \2", src, re.S)
    return [(kernel, expr, sorted(int(v) for v in re.findall(macro + r"\((\d+)\)", body))) for expr, macro, _, kernel, body in found]


def _define(header, name):
    return int(re.search(r"#define %s (\d+)\b" % name, open(os.path.join(CSRC, header)).read()).group(1))


def test_every_compiled_instantiation_is_launched_by_a_case():
    """the count the summary states: 16 / 16 row-pass, 16 / 16 scorer and 8 / 8 gradient-pass instantiations.  A width added to a
    launcher without a case in the lists fails here"""
    tables = {kernel: (expr, labels) for kernel, expr, labels in _dispatch_tables()}
    assert sorted(tables) == ["gauss_score_kernel", "logreg_grad_launch", "logreg_rows_kernel"]
    dims = {"logreg_rows_kernel": [c[2] for c in F.LOGREG_WIDTH_CASES], "logreg_grad_launch": [c[2] for c in F.LOGREG_WIDTH_CASES],
            "gauss_score_kernel": [c[1] for c in F.GAUSS_WIDTH_CASES]}
    onehot = {"logreg_rows_kernel": [c[0] for c in F.ONEHOT_LOGREG_CASES], "logreg_grad_launch": [c[0] for c in F.ONEHOT_LOGREG_CASES],
              "gauss_score_kernel": [c[0] for c in F.ONEHOT_GAUSS_CASES]}
    for kernel, (expr, labels) in tables.items():
        pick = lambda d: eval(expr.replace("/", "//"), {"dim": d})       # the launcher's own expression, in integers
        assert labels == list(range(1, len(labels) + 1)) and len(labels) == {"logreg_grad_launch": 8}.get(kernel, 16), (kernel, labels)
        for lists in (dims, onehot):                                      # the accuracy sweep and the one-hot sweep each reach all
            assert sorted({pick(d) for d in lists[kernel]}) == labels, (kernel, expr)
    # the restated form of the two expressions (the summary's count) agrees with the source's
    assert F.launched_instantiations(F.WIDTHS) == F.compiled_instantiations() == (tables["gauss_score_kernel"][1], tables["logreg_grad_launch"][1])
    assert (F.MIN_DIM, F.MAX_DIM) == (_define("ivit_logreg.h", "LOGREG_MIN_DIM"), _define("ivit_logreg.h", "LOGREG_MAX_DIM")) \
        == (_define("ivit_gauss.h", "GAUSS_MIN_DIM"), _define("ivit_gauss.h", "GAUSS_MAX_DIM"))


def test_width_lists_hold_the_shapes_and_part_counts_they_are_meant_to():
    assert [c[2] for c in F.LOGREG_WIDTH_CASES] == F.WIDTHS == [c[1] for c in F.GAUSS_WIDTH_CASES[:16]] and len(F.WIDTHS) == 16
    assert all(c[:2] == (129, 33) for c in F.LOGREG_WIDTH_CASES) and all((c[0], c[2], c[3]) == (129, 32, 33) for c in F.GAUSS_WIDTH_CASES[:16])
    assert [c[:4] for c in F.GAUSS_WIDTH_CASES[16:]] == [(129, 384, 384, 33), (129, 768, 768, 33)]
    for cus in (1, 256, 304):
        parts = [F.logreg_layout(N, dim, C, splits, cus)["parts"] for N, C, dim, splits, _ in F.LOGREG_WIDTH_CASES]
        assert 1 in parts and 5 in parts and max(parts) == 5           # one part; splits = 9 over five 32-row steps: a part per step
    # the scorer's parts (gauss_shape_bad): per = ceil(tiles / min(want, tiles)), parts = ceil(tiles / per)
    parts = []
    for N, dim, R, C, splits, _ in F.GAUSS_WIDTH_CASES:
        tiles = R // 32 + (C + 31) // 32
        want = splits if splits > 0 else min(256, (2 * 256 + 1) // 2)   # the library's choice on 256 CUs at two row blocks
        per = -(-tiles // min(want, tiles))
        parts.append((-(-tiles // per), tiles, splits))
    assert any(p == 1 for p, _, _ in parts) and any(p == t and s > t for p, t, s in parts) and (14, 14, 16) in parts


@pytest.mark.parametrize("case", F.GAUSS_WIDTH_CASES, ids=str)
def test_gauss_seeds_leave_the_class_to_the_reference(case):
    """the suites compare `cls` only where the float64 top-two gap exceeds 1e-5 max|s| and want 99 % of the rows compared: the
    reference alone meets that on every case of the list"""
    N, dim, R, C, splits, seed = case
    x, Wh, t, Wc, bc = F.gauss_arrays(N, dim, R, C, seed)
    s = x.astype(np.float64) @ Wc.astype(np.float64).T + bc.astype(np.float64)
    top = np.sort(s, axis=1)
    assert ((top[:, -1] - top[:, -2]) > 1e-5 * np.abs(s).max()).mean() >= 0.99


@pytest.mark.parametrize("case", F.LOGREG_WIDTH_CASES + F.LOGREG_FLUSH_CASES, ids=str)
def test_logreg_seeds_leave_correct_to_the_reference(case):
    """`correct` is asserted exactly: on every row the label's logit is further than 1e-5 max|z| from the largest other logit, ten
    times what fp32 accumulation moves a logit by, so whether a row counts as correct is decided in float64 alone"""
    N, C, dim, splits, seed = case
    x, lab, W, b, s = F.logreg_case(N, C, dim, seed)
    z = np.float64(np.float32(s)) * (x.astype(np.float64) @ W.astype(np.float64).T) + b.astype(np.float64)
    zl = z[np.arange(N), lab].copy()
    z[np.arange(N), lab] = -np.inf
    assert np.abs(zl - z.max(axis=1)).min() > 1e-5 * max(np.abs(zl).max(), np.abs(z[np.isfinite(z)]).max())


def test_part_arithmetic_on_both_sides_of_the_flush_limit():
    """float_cases.logreg_layout is logreg_shape_bad (csrc/ivit_hip.hip) restated; the constants are read from csrc/ivit_logreg.h"""
    assert [_define("ivit_logreg.h", n) for n in ("LOGREG_TILE", "LOGREG_PIECES", "LOGREG_ROW_BYTES", "LOGREG_FLUSH_ROWS")] \
        == [F.LOGREG_TILE, F.LOGREG_PIECES, F.LOGREG_ROW_BYTES, F.LOGREG_FLUSH_ROWS]
    assert [c[:4] for c in F.LOGREG_FLUSH_CASES] == [(65536, 33, 64, 1), (65537, 33, 64, 1), (65537, 33, 64, 0)]
    for cus in (0, 1, 64, 256, 304, 2048):
        one, two, lib = (F.logreg_layout(N, dim, C, splits, cus) for N, C, dim, splits, _ in F.LOGREG_FLUSH_CASES)
        assert (one["parts"], one["per"]) == (1, 65536)                 # exactly the limit: one part, as asked
        assert (two["parts"], two["per"]) == (2, 32800)                 # one row more: two parts although one was asked for,
        assert 65537 - 32800 == 32737 and 32737 % 32 == 1               # the second ragged: 1023 whole steps and one row
        # the library's choice: at least the two forced parts, none longer than the limit, and never fewer parts on the device
        # than rows need (on 256 CUs and two class tiles: 256 parts asked, 288 rows each, 228 parts)
        assert lib["parts"] >= 2 and lib["per"] <= F.LOGREG_FLUSH_ROWS and lib["per"] % 32 == 0 and lib["parts"] * lib["per"] >= 65537
        for l in (one, two, lib):
            cpad = 64
            assert l["bytes"] == cpad * 64 * 6 + (65536 if l is one else 65537) * 16 + l["parts"] * cpad * 64 * 4 + l["parts"] * cpad * 4
    assert F.logreg_layout(65537, 64, 33, 0, 256) == dict(tiles=2, parts=228, per=288, bytes=F.logreg_layout(65537, 64, 33, 0, 256)["bytes"])
    # what the size query states (cus = 0) is never less than any device's layout needs
    for N, C, dim, splits, _ in F.LOGREG_FLUSH_CASES + F.LOGREG_WIDTH_CASES:
        assert all(F.logreg_layout(N, dim, C, splits, 0)["bytes"] >= F.logreg_layout(N, dim, C, splits, cus)["bytes"] for cus in (1, 8, 64, 256, 304, 1024, 4096))
    # a part never exceeds the limit, whatever is asked for
    for N in (1, 65535, 65536, 65537, 131072, 131073, 10 ** 7):
        for splits in (0, 1, 2, 3, 4096):
            l = F.logreg_layout(N, 64, 33, splits, 256)
            assert l["per"] <= F.LOGREG_FLUSH_ROWS and (l["parts"] - 1) * l["per"] < N <= l["parts"] * l["per"], (N, splits, l)


def _pieces(w):
    """logreg_split3 in numpy: the leading 16 bits of three floats that sum to w exactly"""
    p0 = (w.view(np.uint32) & 0xFFFF0000).view(np.float32)
    r1 = w - p0
    p1 = (r1.view(np.uint32) & 0xFFFF0000).view(np.float32)
    r2 = r1 - p1
    return p0, p1, (r2.view(np.uint32) & 0xFFFF0000).view(np.float32), r2


def test_one_hot_construction():
    """every weight has three nonzero bf16 pieces that sum to it, all normal; the exponents of one 32-row tile span 2^-30 .. 2^30;
    rows of a tile fall into different pair-steps and both 16-feature halves; over the cases every column position of a 64-feature
    step and every step of every width holds a weight; the features under a weight are powers of two"""
    for dim, R, _ in F.ONEHOT_GAUSS_CASES:
        x, Wh, t, Wc, bc = F.onehot_case(dim, R)
        wrows, wcols, ccols = F.onehot_columns(dim, R)
        assert (np.count_nonzero(Wc, axis=1) == 1).all() and np.count_nonzero(Wh) == R // 32 and not t.any()
        assert all(np.count_nonzero(Wh[i:i + 32]) == 1 for i in range(0, R, 32))
        assert sorted(np.flatnonzero(np.isneginf(bc))) == list(F.ONEHOT_MINUS_INF) and not bc[np.isfinite(bc)].any()
        w = np.concatenate([Wc[np.arange(F.ONEHOT_C), ccols], Wh[wrows, wcols]])
        p0, p1, p2, r2 = _pieces(w)
        assert np.array_equal(p2, r2) and np.array_equal((p0.astype(np.float64) + p1) + p2, w.astype(np.float64))
        assert all((np.abs(p) >= 2.0 ** -126).all() for p in (p0, p1, p2))           # nonzero and normal in bf16
        expo = np.frexp(Wc[np.arange(F.ONEHOT_C), ccols])[1] - 1
        for tile in range(0, 64, 32):
            assert expo[tile:tile + 32].min() <= -27 and expo[tile:tile + 32].max() >= 27 and expo.min() == -30 and expo.max() == 30
            cols = ccols[tile:tile + 32]
            assert len(set(cols // 32)) >= min(8, dim // 32) and set((cols // 16) % 2) == {0, 1}
        assert set(ccols % 64) == set(range(64)) and set(ccols // 64) == set(range(dim // 64))
        under = x[:, np.union1d(wcols, ccols)].astype(np.int64)
        assert ((np.abs(under) & (np.abs(under) - 1)) == 0).all() and (under != 0).all() and set(np.unique(np.abs(under))) == {1, 2, 4, 8, 16, 32, 64, 128}
        rest = np.delete(x, np.union1d(wcols, ccols), axis=1)
        assert rest.size == 0 or len(np.unique(rest)) > 200                                # arbitrary int8 under the zero weights


@pytest.mark.parametrize("dim,R,splits", F.ONEHOT_GAUSS_CASES, ids=str)
def test_one_hot_expectation_equals_the_float64_reference(dim, R, splits):
    """R = 32 is one tile: one rounding (the square), so the float32 expectation is the float64 statement rounded once; `dist` is a
    second rounding (q, then q - best) and may differ from the once-rounded float64 difference by one unit in the last place.
    At R = 96 q adds three rounded squares: checked against float64 to the three roundings"""
    x, *model = F.onehot_case(dim, R)
    dist, cls, q, best = F.onehot_gauss_expected(x, *model)
    wd, wc, wq, wb = gauss_score_reference(x, *model)
    assert all(a.dtype == np.float32 for a in (dist, q, best)) and cls.dtype == np.int32
    assert np.array_equal(cls, wc) and np.array_equal(best, wb.astype(np.float32)) and np.array_equal(best.astype(np.float64), wb)
    assert not np.isin(cls, F.ONEHOT_MINUS_INF).any() and len(np.unique(cls)) > 1 and np.isfinite(dist).all()
    if R == 32:
        assert np.array_equal(q, wq.astype(np.float32))
        assert (np.abs(dist.astype(np.float64) - wd.astype(np.float32)) <= np.spacing(np.abs(wd.astype(np.float32)))).all()
    else:
        assert (np.abs(q - wq) <= 3 * 2.0 ** -24 * wq).all()


@pytest.mark.parametrize("dim,splits", F.ONEHOT_LOGREG_CASES, ids=str)
def test_one_hot_logits_are_exact_in_float32(dim, splits):
    x, lab, W, b, s = F.onehot_logreg_case(dim)
    z64 = np.float64(s) * (x.astype(np.float64) @ W.astype(np.float64).T)
    z32 = np.float32(s) * (W[np.arange(len(W)), np.argmax(W != 0, axis=1)][None, :] * x[:, np.argmax(W != 0, axis=1)].astype(np.float32))
    assert z32.dtype == np.float32 and np.array_equal(z32.astype(np.float64), z64) and not b.any()
    correct = logreg_reference(x, lab, W, b, s)[3]
    assert correct[0] == len(x) and 0 < correct[1] < len(x)
