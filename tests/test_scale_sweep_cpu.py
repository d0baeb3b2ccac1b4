"""The CPU oracle, the CPU twin and the host table builders against the reference swept over activation scales and
requant multipliers (tests/golden/scale_sweep.npz, recorded by tools/make_scale_sweep_fixture.py from the reference's own
modules).  tests/golden/ops.npz pins each operator at a handful of scales with random data; here every operator whose fp32
sequence depends on the scale runs at about 150 scales (48 for I-LayerNorm, 63 for the attention tables) on input blocks
that cover its domain.  CPU only; tests/test_scale_sweep_gpu.py runs the HIP library over the same fixture."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden

import ivit_amd as iv
from ivit_amd import _lib
from oracle import oracle as orc
import scale_sweep as sw
from abi_cases import load_twin

_P = ctypes.c_void_p
UNSUPPORTED = _lib.IVIT_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def g():
    z = load_golden("scale_sweep.npz")
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def twin():
    return load_twin()


def hp(a):
    return a.ctypes.data_as(_P)


def dyv(d):
    return _lib.Dyadic(float(d[0, 0]), float(d[0, 1]))


def check(got, want_csum, what, scale, ref=None):
    """checksum first; on a mismatch name the operator, the scale and how many elements differ from `ref()`"""
    if sw.csum(got) == want_csum:
        return
    n = "?" if ref is None else int((np.asarray(got).astype(np.int64) != np.asarray(ref()).astype(np.int64)).sum())
    raise AssertionError(f"{what} at scale {float(scale)!r}: checksum differs from the reference; {n} of {np.size(got)} "
                         "elements differ from the kept output / oracle")


def test_input_blocks_follow_their_rules(g):
    for n in sw.SHIFTMAX_N:
        x = sw.shiftmax_rows(n)
        assert np.array_equal(x, g[f"shiftmax/{n}/x"])
        assert np.array_equal(x[:256].max(axis=1), np.arange(256) - 128)
    assert all(np.unique(r).size == 256 for r in sw.shiftmax_rows(260)[:256][255:])       # row max 127 holds all 256 values
    x, mask = sw.masked_rows()
    assert np.array_equal(x, g["masked/x"]) and np.array_equal(mask, g["masked/mask"])
    assert np.array_equal(mask, orc.swin_attn_mask(14, 7, 3))
    assert np.array_equal(sw.gelu_block(), g["gelu/x"])
    for C in sw.LN_C:
        x, w, b = sw.ln_block(C)
        assert np.array_equal(x, g[f"ln/{C}/x"]) and np.array_equal(w, g[f"ln/{C}/w"]) and np.array_equal(b, g[f"ln/{C}/b"])
        assert np.ptp(x[-2]) == 0 and set(x[-1].tolist()) == {32767, -32768} and w[0] == np.float32(0.003) and w[1] == -0.5
    assert np.array_equal(sw.qin_grid(), g["qin/grid"])
    for zname, zmax in sw.RQ_ZMAX.items():
        r = sw.rq_ratios(zmax)
        assert np.array_equal(r, g[f"rq/{zname}/ratios"]) and np.array_equal(sw.rq_block(zmax, r), g[f"rq/{zname}/z"])
        a = np.abs(r.astype(np.float64))
        assert a.min() < 2.0 ** -28 and a.max() >= 2.0 ** 12
        for b in (512.0, 1024.0, 2048.0, 2.0 ** 31 / zmax):
            assert (a < b).any() and (a > b).any() and np.abs(a / b - 1).min() < 2e-7
    assert np.array_equal(sw.rq_identity(), g["rq/z_id"])
    ew = g["ew/scales"]
    assert ew.size == 150 and ew.min() < 1e-3 and (ew > 1).sum() >= 3
    for v in (0.5, 0.25, 0.125, 0.0625, 0.015625):
        assert np.nextafter(np.float32(v), np.float32(0)) in ew and np.nextafter(np.float32(v), np.float32(1)) in ew


def test_shiftmax_oracle_and_twin(g, twin):
    for n in sw.SHIFTMAX_N:
        x, bits = g[f"shiftmax/{n}/x"], sw.SHIFTMAX_BITS[n]
        sets = [(g["ew/scales"], g[f"shiftmax/{n}/csum"])]
        if bits == 16:
            sets.append((g["attn/scales"], g[f"shiftmax/{n}/attn_csum"]))
        for scales, cs in sets:
            for i, s in enumerate(scales):
                got = orc.shiftmax(x, s, bits)
                check(got, cs[i], f"oracle.shiftmax n={n} bits={bits}", s, lambda: g.get(f"shiftmax/{n}/out/{i}", got))
                out = np.empty(x.shape, np.uint16)
                assert twin.ivit_cpu_shiftmax(None, hp(x), x.shape[0], n, n, float(s), bits, hp(out), n) == 0
                check(out, cs[i], f"ivit_cpu_shiftmax n={n} bits={bits}", s, lambda: got)
        for i in g["ew/full"]:
            if f"shiftmax/{n}/out/{i}" in g:
                assert np.array_equal(orc.shiftmax(x, g["ew/scales"][i], bits), g[f"shiftmax/{n}/out/{i}"]), (n, i)


def test_masked_shiftmax_oracle_and_twin(g, twin):
    x, mask = g["masked/x"], g["masked/mask"]
    rows, n = x.shape
    for i, s in enumerate(g["ew/scales"]):
        got = orc.shiftmax_masked(x, s, 8, mask, sw.MASK_NW, sw.MASK_H)
        check(got, g["masked/csum"][i], "oracle.shiftmax_masked", s, lambda: g.get(f"masked/out/{i}", got))
        out = np.empty(x.shape, np.uint16)
        assert twin.ivit_cpu_shiftmax_masked(None, hp(x), rows, n, n, float(s), 8, hp(mask), sw.MASK_NW, sw.MASK_H, hp(out), n) == 0
        check(out, g["masked/csum"][i], "ivit_cpu_shiftmax_masked", s, lambda: got)
    # mask == NULL is the plain Shiftmax: rows 0..258 of the block are the n = 49 rows
    s = g["ew/scales"][7]
    assert np.array_equal(orc.shiftmax_masked(x[:259], s, 8, None, 1, 1), orc.shiftmax(g["shiftmax/49/x"], s, 8))


def gelu_overflows(g):
    return (g["gelu/min"] < -32768) | (g["gelu/max"] > 32767)


def test_shiftgelu_overflow_regime(g, twin):
    """The product Q*sigmoid_int leaves int16 below a scale that the fixture's recorded extremes locate (about 1.2e-3: the
    reference's clamp of the exponential sum at 2^31 lets sigmoid_int exceed 256).  The 16-bit forms refuse exactly the
    scales that overflow; nothing wraps."""
    ew, over = g["ew/scales"], gelu_overflows(g)
    assert over.any() and not over.all()
    assert np.array_equal(g["gelu/maxabs"], np.maximum(-g["gelu/min"].astype(np.int64), g["gelu/max"]).astype(np.int32))
    threshold = ew[over].max()                       # the largest scale at which the product leaves int16
    assert (ew > threshold).any()
    print(f"Q*sigmoid_int leaves int16 at {int(over.sum())} of {ew.size} scales, the largest {float(threshold)!r}; the "
          f"smallest scale that fits is {float(ew[~over].min())!r}")
    x = g["gelu/x"]
    out = np.empty(x.shape, np.int16)
    for i, s in enumerate(ew):
        lo, hi = orc.shiftgelu_range(s)
        assert (lo, hi) == (int(g["gelu/min"][i]), int(g["gelu/max"][i])), float(s)
        rc = twin.ivit_cpu_shiftgelu(None, hp(x), 256, 256, float(s), hp(out))
        if over[i]:
            assert rc == UNSUPPORTED, float(s)
            with pytest.raises(OverflowError):
                orc.shiftgelu(x, s)
        else:
            assert rc == 0, f"scale {float(s)!r} fits int16 (max |Q*sig| {int(g['gelu/maxabs'][i])}) and was refused"
            check(out, g["gelu/csum"][i], "ivit_cpu_shiftgelu", s)
            assert np.array_equal(orc.shiftgelu(x, s), out)


def test_shiftgelu_oracle_and_twin(g, twin):
    x = g["gelu/x"]
    tri = np.tril(np.ones((256, 256), bool))          # the table entries with Q <= row max
    o8, tab, lut = (np.empty((256, 256), np.int8) for _ in range(3))
    for i, s in enumerate(g["ew/scales"]):
        prod = orc.shiftgelu32(x, s)
        check(prod, g["gelu/csum"][i], "oracle.shiftgelu32", s, lambda: g.get(f"gelu/prod/{i}", prod))
        assert (prod.min(), prod.max()) == (g["gelu/min"][i], g["gelu/max"][i])
        for j in range(2):
            dy = iv.freeze.dyadic(np.float32(s * np.float32(2.0 ** -7)), g["gelu/s_out8"][i, j])
            want = orc.requant(prod, orc.dyadic(np.float32(s * np.float32(2.0 ** -7)), g["gelu/s_out8"][i, j]), 8)
            check(want, g["gelu/csum8"][i, j], "oracle.shiftgelu32 + requant", s, lambda: g.get(f"gelu/out8/{j}/{i}", want))
            assert twin.ivit_cpu_shiftgelu_requant(None, hp(x), 256, 256, float(s), dyv(dy), hp(o8)) == 0
            check(o8, g["gelu/csum8"][i, j], "ivit_cpu_shiftgelu_requant", s, lambda: want)
            assert twin.ivit_cpu_shiftgelu_build_table(None, float(s), dyv(dy), hp(tab)) == 0
            assert np.array_equal(tab[tri], want[tri].astype(np.int8)) and not tab[~tri].any(), float(s)
            assert twin.ivit_cpu_shiftgelu_requant_lut(None, hp(x), 256, 256, hp(tab), hp(lut)) == 0
            check(lut, g["gelu/csum8"][i, j], "ivit_cpu_shiftgelu_requant_lut", s, lambda: want)


def test_layernorm_oracle_and_twin(g, twin):
    s_out = g["ln/s_out"]
    for C in sw.LN_C:
        x = g[f"ln/{C}/x"]
        rows = x.shape[0]
        bias_int, sc = orc.layernorm_consts(g[f"ln/{C}/w"], g[f"ln/{C}/b"], C)
        b2, sc2 = iv.freeze.layernorm_constants(g[f"ln/{C}/w"], g[f"ln/{C}/b"])
        assert np.array_equal(bias_int, b2) and np.array_equal(sc, sc2)
        dy = iv.freeze.dyadic(sc, s_out)
        z2, o8 = np.empty((rows, C), np.float32), np.empty((rows, C), np.int8)
        for i, s in enumerate(g["ln/scales"]):
            z = orc.layernorm(x, s, bias_int, sc)
            check(z.astype(np.float64), g[f"ln/{C}/csum_z"][i], f"oracle.layernorm C={C}", s, lambda: g.get(f"ln/{C}/z/{i}", z))
            out = orc.requant(z, orc.dyadic(sc, s_out), 8)
            check(out, g[f"ln/{C}/csum8"][i], f"oracle.layernorm + requant C={C}", s, lambda: g.get(f"ln/{C}/out8/{i}", out))
            assert twin.ivit_cpu_layernorm(None, hp(x), rows, C, float(s), hp(bias_int), hp(sc), hp(z2)) == 0
            assert np.array_equal(z2, z), (C, float(s))
            assert twin.ivit_cpu_layernorm_requant(None, hp(x), rows, C, C, float(s), hp(bias_int), hp(sc), hp(dy), hp(o8)) == 0
            check(o8, g[f"ln/{C}/csum8"][i], f"ivit_cpu_layernorm_requant C={C}", s, lambda: out)
            for k in (f"ln/{C}/z/{i}", f"ln/{C}/out8/{i}"):
                if k in g:
                    assert np.array_equal(g[k], z if "/z/" in k else out.astype(np.int8)), k


def test_tokenorder_layernorm_oracle_and_twin(g, twin):
    """oracle.layernorm_ord(order=1) — the reference of the GPU token-order kernels — against the reference's IntLayerNorm on
    a token-contiguous input: two images of 49 tokens (one group of 32 tokens and 17 left over per image)"""
    s_out, L = g["ln/s_out"], sw.LN_TOKENS
    for C in sw.LN_TOKEN_C:
        x, w, b = sw.ln_token_block(C)
        rows = x.shape[0]
        bias_int, sc = orc.layernorm_consts(w, b, C)
        dy = iv.freeze.dyadic(sc, s_out)
        z2, o8 = np.empty((rows, C), np.float32), np.empty((rows, C), np.int8)
        differs = 0
        for i, s in enumerate(g["ln/scales"]):
            z = orc.layernorm_ord(x, s, bias_int, sc, 1, L)
            check(z.astype(np.float64), g[f"lntok/{C}/csum_z"][i], f"oracle.layernorm_ord C={C}", s,
                  lambda: g.get(f"lntok/{C}/z/{i}", z))
            out = orc.requant(z, orc.dyadic(sc, s_out), 8)
            check(out, g[f"lntok/{C}/csum8"][i], f"oracle.layernorm_ord + requant C={C}", s)
            differs += int(not np.array_equal(z, orc.layernorm(x, s, bias_int, sc)))
            assert twin.ivit_cpu_layernorm_tokenorder(None, hp(x), rows, C, float(s), hp(bias_int), hp(sc), L, hp(z2)) == 0
            assert np.array_equal(z2, z), (C, float(s))
            assert twin.ivit_cpu_layernorm_tokenorder_requant(None, hp(x), rows, C, float(s), hp(bias_int), hp(sc), hp(dy), L, hp(o8)) == 0
            check(o8, g[f"lntok/{C}/csum8"][i], f"ivit_cpu_layernorm_tokenorder_requant C={C}", s, lambda: out)
        print(f"C={C}: token order changes z at {differs} of {len(g['ln/scales'])} scales")


def test_input_quantisation_oracle_and_twin(g, twin):
    for i, s in enumerate(g["qin/scales"]):
        x = sw.qin_values(s)
        got = orc.quantize_f32(x, s, 8)
        check(got, g["qin/csum"][i], "oracle.quantize_f32", s, lambda: g.get(f"qin/out/{i}", got))
        q = np.empty(x.size, np.int8)
        assert twin.ivit_cpu_quantize_input_f32(None, hp(x), float(s), hp(q), x.size) == 0
        check(q, g["qin/csum"][i], "ivit_cpu_quantize_input_f32", s, lambda: got)
        if i in g["ew/full"]:
            assert got.min() == -128 and got.max() == 127           # saturation at every scale


def test_requant_multiplier_sweep_oracle_and_twin(g, twin):
    zi = g["rq/z_id"]
    for ci, (zname, bits, ident) in enumerate(sw.RQ_CASES):
        z, ratios = g[f"rq/{zname}/z"], g[f"rq/{zname}/ratios"]
        want = g[f"rq/out/{ci}"].astype(np.int32)
        s_pre = (ratios * sw.RQ_S_OUT).astype(np.float32)
        dy, dyi = orc.dyadic(s_pre, sw.RQ_S_OUT), None
        fd, fdi = iv.freeze.dyadic(s_pre, sw.RQ_S_OUT), None
        if ident:
            s_id = np.float32(sw.RQ_ID_RATIO[ident] * sw.RQ_S_OUT)
            dyi, fdi = orc.dyadic(s_id, sw.RQ_S_OUT), iv.freeze.dyadic(s_id, sw.RQ_S_OUT)
        got = orc.requant(z, dy, bits, zi if ident else None, dyi)
        assert np.array_equal(got, want), (ci, zname, bits, ident, ratios[np.unique(np.nonzero(got != want)[1])])
        gotf = orc.requant(z.astype(np.float32), dy, bits, zi.astype(np.float32) if ident else None, dyi)
        assert np.array_equal(gotf, want), ci
        lim = 2 ** (bits - 1)
        sat = (want == lim - 1) | (want == -lim)
        assert 0.05 < sat.mean() < (0.95 if not ident else 1.0), sat.mean()    # saturated in part, not everywhere
        out = np.empty(z.shape, np.int8 if bits == 8 else np.int16)
        idp, didp = (hp(zi), hp(fdi)) if ident else (None, None)
        fns = [("requant_i32", z), ("requant_f32", z.astype(np.float32))] + ([("requant_i16", z.astype(np.int16))] if zname == "z16" else [])
        for name, zz in fns:
            out[:] = 0
            assert getattr(twin, "ivit_cpu_" + name)(None, hp(zz), hp(fd), sw.RQ_C, idp, didp, bits, hp(out), z.shape[0], sw.RQ_C) == 0
            assert np.array_equal(out.astype(np.int32), want), (name, ci)
    # the exact .5 ties are there: a multiplier 2^-k on an odd multiple of 2^(k-1)
    z, r = g["rq/z16/z"], g["rq/z16/ratios"].astype(np.float64)
    frac = np.abs(z * r[None, :]) % 1.0
    assert (frac == 0.5).sum() >= 32


def _shiftmax_from_exps(e):
    """the rest of the Shiftmax arithmetic after exp_int (quant_modules.py:489-493), 16 bit"""
    S = np.array([orc.torch_sum(row) for row in e], np.float32)
    S = np.minimum(S, np.float32(2147483648.0))
    F = np.floor((np.float32(1.0) / S).astype(np.float32) * np.float32(2147483648.0)).astype(np.float32)
    return np.floor(((e * F[:, None]).astype(np.float32)) * np.float32(2.0 ** -16)).astype(np.int64)


def attention_tables(g):
    out = []
    for s in g["attn/scales"]:
        tabs = iv.freeze.shiftmax_tables(s)
        out.append((s, tabs, iv.freeze.shiftmax_rowtable(tabs)))
    return out


def test_shiftmax_tables_reproduce_the_reference(g):
    """freeze.shiftmax_tables and freeze.shiftmax_rowtable, taken through the rest of the Shiftmax arithmetic, give the
    reference's 16-bit Shiftmax at every attention scale that has tables"""
    for i, (s, tabs, rowtab) in enumerate(attention_tables(g)):
        if tabs is None:
            continue
        for n in (17, 197, 260):
            x = g[f"shiftmax/{n}/x"]
            xi = x.astype(np.int64)
            vmax = xi.max(axis=1, keepdims=True)
            dd = np.maximum(xi - vmax, tabs["dmin"]) - tabs["dmin"]
            idx = tabs["aq"][tabs["cls"][vmax[:, 0] + 128]][np.arange(x.shape[0])[:, None], xi + 128].astype(np.int64) + dd
            e = tabs["t"][idx].astype(np.float32)
            check(_shiftmax_from_exps(e), g[f"shiftmax/{n}/attn_csum"][i], f"shiftmax_tables n={n}", s,
                  lambda: orc.shiftmax(x, s, 16))
            if rowtab is not None:
                e2 = rowtab[vmax + 128, dd]
                assert np.array_equal(e2, e), (float(s), n)


def test_attention_scales_cover_every_table_form(g):
    """Coverage conditions of the attention sweep.  A row-table line has R = 1 - dmin entries and R follows x0 = floor(-1/s)
    in steps of about ten (43, 54, 64, 74, 85 for x0 = -4 .. -8), so R = 65 does not occur at any scale: the boundary of
    ivit_shiftmax_rowtable is the pair of adjacent float32 scales around 1/6 with R = 64 and R = 74."""
    t = attention_tables(g)
    n = len(t)
    assert n >= 60
    assert sum(tabs is not None for _, tabs, _ in t) * 2 >= n
    assert sum(rt is not None for _, _, rt in t) * 3 >= n
    R = {float(s): tabs["R"] for s, tabs, _ in t if tabs is not None}
    assert 64 in R.values() and any(tabs is None for _, tabs, _ in t)
    over = min(r for r in R.values() if r > 64)
    lo = max(s for s, r in R.items() if r == over)
    hi = min(s for s, r in R.items() if r == 64)
    assert np.float32(hi) == np.nextafter(np.float32(lo), np.float32(1)), (lo, hi, over)     # nothing lies between them
    assert all(rt is None for _, tabs, rt in t if tabs is not None and tabs["R"] > 64)
