"""Both sides of every 32-bit size limit in the launchers, on the device: one allocation, one launch and a chunked comparison of EVERY
byte per case of tests/large_cases.py (the table of size decisions is that module's docstring).  The expected output is the CPU
oracle's answer for a small block, repeated; the large input is the block repeated on the device, the last repeat cut at M.  Every
output lies between two 4 KiB guards that must be intact afterwards.  A case that finds less than its bytes plus 1 GiB free skips with
both numbers in the reason; a skip is not a pass."""
import ctypes
import functools
import gc
import time

import numpy as np
import pytest

from conftest import load_golden, golden_scales

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402
import large_cases as lc  # noqa: E402
import scale_sweep as sw  # noqa: E402

_P = ctypes.c_void_p
G, FILL = lc.GUARD_BYTES, lc.FILL
FILL8 = int(np.array([FILL], np.uint8).view(np.int8)[0])        # the fill as an int8 value
S_IN, S_LN = np.float32(7.3e-4), np.float32(0.031)                                      # a LayerNorm: scale of its 16-bit input, of its 8-bit output
S_MID, S_FIN, S_RES = np.float32(2e-4), np.float32(3.1e-4), np.float32(2.7e-4)          # a residual QuantAct: qact, output, identity branch
UNSUPPORTED, INVALID = _lib.IVIT_ERR_UNSUPPORTED, 1


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


_KEEP = []


@pytest.fixture(autouse=True)
def _free_between_cases():
    yield
    del _KEEP[:]
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def P(t):
    return _P(t.data_ptr())


def dev(a):
    """host -> device; the tensor is kept alive until the case ends (raw pointers are handed to the C-ABI)"""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    _KEEP.append(t)
    return t


def dyv(d):
    """an ivit_dyadic by value, from iv.freeze.dyadic's [1, 2] array or the oracle's Dyadic array"""
    return _lib.Dyadic(float(d[0, 0]), float(d[0, 1])) if isinstance(d, np.ndarray) else _lib.Dyadic(float(d[0].m), float(d[0].r))


def status(H, name, *args):
    return getattr(H.lib, name)(H.h, *args)


def err(H):
    return H.lib.ivit_last_error(H.h).decode()


def begin(cid):
    """the case, after the look at the device's free memory; the clock of the case starts here"""
    c = lc.BY_ID[cid]
    need = c.bytes + lc.GIB
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"{free} bytes free on the device, {need} needed")
    c.t0 = time.time()
    return c


def done(c, what=""):
    torch.cuda.synchronize()
    print(f"LARGE {c.id}: {c.bytes} device bytes, {time.time() - c.t0:.2f} s, {c.kernel} {what}")


def rep(block, M):
    """[M, ...] on the device whose row r is block[r % p]"""
    return lc.repeat_rows(torch, dev(block), M)


class Buf:
    """`nbytes` of payload between two 4 KiB guards, everything filled with 0x5A (guarded() of tests/test_search_gpu.py)"""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.whole = torch.full((G + self.n + G,), FILL, dtype=torch.uint8, device="cuda")
        self.bytes = self.whole[G:G + self.n]

    def view(self, dtype, *shape):
        return self.bytes.view(dtype).view(*shape)

    def intact(self):
        return bool((self.whole[:G] == FILL).all()) and bool((self.whole[G + self.n:] == FILL).all())

    def untouched(self):
        return lc.all_equal_to(torch, self.bytes, FILL)


def expect(buf, dtype, want, M):
    """the whole of `buf`, as [M, width of want] of `dtype`, equals want[r % p] in every row r, and the guards are intact"""
    torch.cuda.synchronize()
    assert buf.intact(), "wrote outside its output"
    want = np.ascontiguousarray(want).reshape(want.shape[0], -1)
    if want.dtype == np.uint16:
        want = want.view(np.int16)
    if want.dtype == np.float32:
        want = want.view(np.int32)
    wd = dev(want)
    W = want.shape[1]
    assert buf.n == M * W * want.itemsize, (buf.n, M, W, want.itemsize)
    row = lc.first_mismatch(torch, buf.view(wd.dtype, M, W), wd)
    assert row is None, lc.where_it_is(row, W, want.itemsize)


# ---------------------------------------------------------------- host blocks and their oracle answers: computed once, left unchanged
def orc():
    from oracle import oracle
    return oracle


@functools.lru_cache(maxsize=None)
def layer(N, K, bits):
    """a frozen QuantLinear K -> N with an 8- or 16-bit QuantAct behind it (the recipe of tests/test_ws192_gpu.py): the accumulators'
    standard deviation at 0.4 of the output range, so that both clamps are reached"""
    rng = np.random.default_rng(N * 4 + bits + K)
    w = np.rint(rng.normal(0, 45, (N, K)).clip(-128, 127)).astype(np.int8)
    b = rng.integers(-2 ** 14, 2 ** 14, N).astype(np.int32)
    s_pre = (10 ** rng.uniform(-5.5, -5, N)).astype(np.float32)
    s_out = np.float32(45.0 * 74.0 * np.sqrt(K) * float(np.abs(s_pre).mean()) / (0.4 * 2 ** (bits - 1)))
    return w, b, s_pre, s_out


@functools.lru_cache(maxsize=None)
def rows8(p, K, seed=0):
    return np.random.default_rng(1000 * p + K + seed).integers(-128, 128, (p, K), dtype=np.int8)


@functools.lru_cache(maxsize=None)
def rows16(p, N, seed=0):
    """identity rows over the whole 16-bit range, row 0 alternating the two ends"""
    res = np.random.default_rng(2000 * p + N + seed).integers(-32768, 32768, (p, N)).astype(np.int16)
    res[0, 0::2], res[0, 1::2] = 32767, -32768
    return res


@functools.lru_cache(maxsize=None)
def norm_consts(C):
    """LayerNorm constants with negative gammas among them"""
    rng = np.random.default_rng(193 + C)
    wln = rng.normal(1.0, 0.4, C).astype(np.float32)
    wln[1] = -0.5
    return iv.freeze.layernorm_constants(wln, rng.normal(0.0, 0.5, C).astype(np.float32))


@functools.lru_cache(maxsize=None)
def tokens16(p, C):
    """16-bit LayerNorm input [p, C] (half of the channels small, row 1 constant: zero variance) and the oracle's norm + qact(8) of it"""
    rng = np.random.default_rng(7 * p + C)
    x16 = rng.integers(-26000, 26000, (p, C)).astype(np.int16)
    x16[:, : C // 2] //= 64
    x16[1] = 1234
    bias_int, sc = norm_consts(C)
    ln8 = orc().requant(orc().layernorm(x16, float(S_IN), bias_int, sc), orc().dyadic(sc, S_LN), 8).astype(np.int8)
    return x16, ln8


@functools.lru_cache(maxsize=None)
def linear_want(p, N, K, bits, ln=False):
    """(input block, oracle's Linear + QuantAct(bits) of it [p, N] int32); ln: the input is tokens16's norm output"""
    w, b, s_pre, s_out = layer(N, K, bits)
    x = tokens16(p, K)[1] if ln else rows8(p, K)
    return x, orc().requant(orc().linear_i8(x, w, b), orc().dyadic(s_pre, s_out), bits)


@functools.lru_cache(maxsize=None)
def residual_want(p, N, K):
    """(x, identity rows, oracle's Linear -> QuantAct(16) -> residual QuantAct [p, N] int32)"""
    x, t = linear_want(p, N, K, 16)
    res = rows16(p, N)
    return x, res, orc().requant(t, orc().dyadic(S_MID, S_FIN), 16, res.astype(np.int32), orc().dyadic(S_RES, S_FIN))


class Layer:
    """device copies of a layer, its plan (prepared for the weights-in-registers kernel or not) and the LayerNorm constants"""

    def __init__(self, H, N, K, bits, prepared=False):
        w, b, s_pre, s_out = layer(N, K, bits)
        self.w, self.b, self.d = dev(w), dev(b), dev(iv.freeze.dyadic(s_pre, s_out))
        self.plan = H.linear_plan(P(self.w), P(self.b), P(self.d), N, K)
        assert self.plan.pipelined_ok
        if prepared:
            H.call("ivit_linear_plan_prepare_ws", self.plan.p)

    def close(self):
        self.plan.close()


def ln_dev(C):
    bias_int, sc = norm_consts(C)
    return dev(bias_int), dev(sc), dev(iv.freeze.dyadic(sc, S_LN))


# ---------------------------------------------------------------- planned GEMMs
@pytest.mark.parametrize("cid", lc.ids("planned_requant"))
def test_planned_requant(H, cid):
    c = begin(cid)
    M, N, K, bits = (c.sizes[k] for k in ("M", "N", "K", "bits"))
    assert lc.requant_planned_route(False, M, N, K, bits) == c.kernel
    xb, want = linear_want(c.period, N, K, bits)
    L = Layer(H, N, K, bits)
    try:
        x, out = rep(xb, M), Buf(M * N * bits // 8)
        H.call("ivit_linear_i8_requant_planned", L.plan.p, P(x), bits, P(out.bytes), M)
        expect(out, None, want.astype(np.int8 if bits == 8 else np.int16), M)
        assert want.min() == -2 ** (bits - 1) and want.max() == 2 ** (bits - 1) - 1
    finally:
        L.close()
    done(c)


@pytest.mark.parametrize("cid", lc.ids("planned_residual"))
def test_planned_residual(H, cid):
    c = begin(cid)
    M, N, K = (c.sizes[k] for k in ("M", "N", "K"))
    assert lc.residual_planned_route(False, M, N, K) == c.kernel
    xb, resb, want = residual_want(c.period, N, K)
    L = Layer(H, N, K, 16)
    try:
        x, res, out = rep(xb, M), rep(resb, M), Buf(M * N * 2)
        H.call("ivit_linear_i8_requant_residual_planned", L.plan.p, P(x), dyv(iv.freeze.dyadic(S_MID, S_FIN)), dyv(iv.freeze.dyadic(S_RES, S_FIN)),
               P(res), P(out.bytes), M)
        expect(out, None, want.astype(np.int16), M)
        assert len(np.unique(want)) > 1000
    finally:
        L.close()
    done(c)


@functools.lru_cache(maxsize=None)
def qkv_want(pi, T, H_, dh, ln):
    """(input block [pi * T, D], [3][pi, H, T, dh] int8: the oracle's qkv Linear + QuantAct(8) scattered as the entry scatters it)"""
    D = H_ * dh
    x, want = linear_want(pi * T, 3 * D, D, 8, ln)
    src = tokens16(pi * T, D)[0] if ln else x
    return src, np.ascontiguousarray(want.astype(np.int8).reshape(pi, T, 3, H_, dh).transpose(2, 0, 3, 1, 4))


@pytest.mark.parametrize("cid", lc.ids("planned_qkv"))
def test_planned_qkv(H, cid):
    """ivit_linear_i8_qkv_planned and its norm1-headed form: q, k [B * H, T, dh], v the same (ldv = 0) or v^T [B * H * dh, ldv] of which
    only the columns t < T are written"""
    c = begin(cid)
    B, T, H_, dh, ldv, prepared, ln = (c.sizes[k] for k in ("B", "T", "H", "dh", "ldv", "prepared", "ln"))
    D, pi = H_ * dh, c.period
    refused = c.kernel == "IVIT_ERR_UNSUPPORTED"
    assert lc.qkv_ws_ok(prepared, D, 3 * D, B, T, H_, dh, ldv) == (not refused) if ln else lc.qkv_planned_route(prepared, B, T, H_, dh, ldv) == c.kernel
    src, want = qkv_want(pi, T, H_, dh, ln)
    L = Layer(H, 3 * D, D, 8, prepared)
    try:
        x = rep(src.reshape(pi, T * D), B)
        q, k = Buf(B * H_ * T * dh), Buf(B * H_ * T * dh)
        v = Buf(B * H_ * T * dh if ldv == 0 else B * H_ * dh * ldv)
        if ln:
            bi, sc, dln = ln_dev(D)
            st = status(H, "ivit_layernorm_linear_i8_qkv_ldv_planned", L.plan.p, P(x), float(S_IN), P(bi), P(sc), P(dln), P(q.bytes), P(k.bytes),
                        P(v.bytes), B, T, H_, dh, ldv)
        else:
            st = status(H, "ivit_linear_i8_qkv_planned", L.plan.p, P(x), P(q.bytes), P(k.bytes), P(v.bytes), B, T, H_, dh, ldv)
        torch.cuda.synchronize()
        if refused:
            assert st == UNSUPPORTED and "2^31" in err(H), (st, err(H))
            assert q.untouched() and k.untouched() and v.untouched() and q.intact() and k.intact() and v.intact()
        else:
            assert st == 0, err(H)
            expect(q, None, want[0].reshape(pi, -1), B)
            expect(k, None, want[1].reshape(pi, -1), B)
            if ldv == 0:
                expect(v, None, want[2].reshape(pi, -1), B)
            else:
                assert v.intact(), "wrote outside v^T"
                vt = v.view(torch.int8, B, H_ * dh, ldv)
                wt = dev(want[2].transpose(0, 1, 3, 2).reshape(pi, H_ * dh * T))       # [pi, H * dh, T]: element (h, ch, t)
                row = lc.first_mismatch(torch, vt[:, :, :T].reshape(B, H_ * dh * T), wt)
                assert row is None, f"v^T: first differing image {row}"
                rows_per = max(1, lc.CHUNK_BYTES // ldv)
                flat = vt.view(B * H_ * dh, ldv)
                for r0 in range(0, B * H_ * dh, rows_per):
                    assert bool((flat[r0:r0 + rows_per, T:] == FILL8).all()), f"v^T columns t >= T written in rows {r0} .. {r0 + rows_per}"
            assert want.min() == -128 and want.max() == 127
    finally:
        L.close()
    done(c, f"status {st}")


@pytest.mark.parametrize("cid", lc.ids("planned_ln_requant"))
def test_planned_layernorm_requant(H, cid):
    c = begin(cid)
    M, N, K = (c.sizes[k] for k in ("M", "N", "K"))
    assert lc.ws_plan_ok(True, K, M)
    _, want = linear_want(c.period, N, K, 8, True)
    L = Layer(H, N, K, 8, prepared=True)
    try:
        x16, out = rep(tokens16(c.period, K)[0], M), Buf(M * N)
        bi, sc, dln = ln_dev(K)
        H.call("ivit_layernorm_linear_i8_requant_planned", L.plan.p, P(x16), float(S_IN), P(bi), P(sc), P(dln), P(out.bytes), M)
        expect(out, None, want.astype(np.int8), M)
    finally:
        L.close()
    done(c)


@pytest.mark.parametrize("cid", lc.ids("planned_residual_ln"))
def test_planned_residual_layernorm(H, cid):
    c = begin(cid)
    M, N, K = (c.sizes[k] for k in ("M", "N", "K"))
    assert lc.ws_plan_ok(True, K, M) and N == K == 384
    xb, resb, want = residual_want(c.period, N, K)
    bias_int, scn = norm_consts(K)
    want8 = orc().requant(orc().layernorm(want.astype(np.int16), float(S_FIN), bias_int, scn), orc().dyadic(scn, S_LN), 8)
    L = Layer(H, N, K, 16, prepared=True)
    try:
        x, res, out, o8 = rep(xb, M), rep(resb, M), Buf(M * N * 2), Buf(M * N)
        bi, sc, dln = ln_dev(K)
        H.call("ivit_linear_i8_requant_residual_layernorm_planned", L.plan.p, P(x), dyv(iv.freeze.dyadic(S_MID, S_FIN)),
               dyv(iv.freeze.dyadic(S_RES, S_FIN)), P(res), P(out.bytes), M, float(S_FIN), P(bi), P(sc), P(dln), P(o8.bytes))
        expect(out, None, want.astype(np.int16), M)
        expect(o8, None, want8.astype(np.int8), M)
    finally:
        L.close()
    done(c)


# ---------------------------------------------------------------- kernels with no predicate
@pytest.mark.parametrize("cid", lc.ids("requant_i32"))
def test_requant_i32(H, cid):
    c = begin(cid)
    rows, C, bits = (c.sizes[k] for k in ("rows", "C", "bits"))
    rng = np.random.default_rng(C)
    zb = rng.integers(-2 ** 20, 2 ** 20, (c.period, C)).astype(np.int32)
    zb[0], zb[1] = 2 ** 20, -2 ** 20
    s_pre, s_out = np.float32(1.0e-4), np.float32(1.0e-4 * 0.7 * 2 ** 20 / 2 ** (bits - 1))      # the largest |z| lands at 1.43 of the range
    want = orc().requant(zb, orc().dyadic(s_pre, s_out), bits)
    assert want.min() == -2 ** (bits - 1) and want.max() == 2 ** (bits - 1) - 1
    z, out = rep(zb, rows), Buf(rows * C * bits // 8)
    H.call("ivit_requant_i32", P(z), P(dev(iv.freeze.dyadic(s_pre, s_out))), 1, None, None, bits, P(out.bytes), rows, C)
    expect(out, None, want.astype(np.int8 if bits == 8 else np.int16), rows)
    done(c)


@pytest.mark.parametrize("cid", lc.ids("quantize_input"))
def test_quantize_input(H, cid):
    c = begin(cid)
    n, scale = c.sizes["n"], np.float32(0.0207)
    rng = np.random.default_rng(5)
    grid = sw.qin_values(scale)                                   # ties, near-ties and saturation
    xb = np.concatenate([grid, rng.normal(0, 1.5, c.period - grid.size).astype(np.float32)])[:, None]
    want = orc().quantize_f32(xb, float(scale), 8).astype(np.int8)
    x, q = rep(xb, n), Buf(n)
    H.call("ivit_quantize_input_f32", P(x), float(scale), P(q.bytes), n)
    expect(q, None, want, n)
    done(c)


@pytest.mark.parametrize("cid", lc.ids("widen"))
def test_widen(H, cid):
    c = begin(cid)
    n = c.sizes["n"]
    xb = rows8(c.period, 1)
    x, out = rep(xb, n), Buf(n * 2)
    H.call("ivit_widen_i8_i16", P(x), P(out.bytes), n)
    expect(out, None, xb.astype(np.int16), n)
    done(c)


@pytest.mark.parametrize("cid", lc.ids("layernorm_requant"))
def test_layernorm_requant(H, cid):
    c = begin(cid)
    rows, C = c.sizes["rows"], c.sizes["C"]
    x40, w, b = sw.ln_block(C)                                    # amplitudes 2 .. 30 000, a zero-variance row, an alternating row
    xb = np.concatenate([x40, tokens16(c.period - x40.shape[0], C)[0]])
    bias_int, sc = iv.freeze.layernorm_constants(w, b)
    want = orc().requant(orc().layernorm(xb, float(S_IN), bias_int, sc), orc().dyadic(sc, S_LN), 8)
    x, out = rep(xb, rows), Buf(rows * C)
    H.call("ivit_layernorm_requant", P(x), rows, C, C, float(S_IN), P(dev(bias_int)), P(dev(sc)), P(dev(iv.freeze.dyadic(sc, S_LN))), P(out.bytes))
    expect(out, None, want.astype(np.int8), rows)
    assert len(np.unique(want)) > 50
    done(c)


@pytest.mark.parametrize("cid", lc.ids("layernorm_tokenorder"))
def test_layernorm_tokenorder(H, cid):
    """the token-order sums depend on a row's position in its image: the block is whole images"""
    c = begin(cid)
    B, L, C = c.sizes["B"], c.sizes["L"], c.sizes["C"]
    x40, w, b = sw.ln_block(C)
    rows_b = c.period * L
    xb = np.concatenate([x40, tokens16(rows_b - x40.shape[0], C)[0]])
    bias_int, sc = iv.freeze.layernorm_constants(w, b)
    want = orc().requant(orc().layernorm_ord(xb, float(S_IN), bias_int, sc, 1, L), orc().dyadic(sc, S_LN), 8)
    rows = B * L
    x, out = rep(xb, rows), Buf(rows * C)
    H.call("ivit_layernorm_tokenorder_requant", P(x), rows, C, float(S_IN), P(dev(bias_int)), P(dev(sc)), P(dev(iv.freeze.dyadic(sc, S_LN))), L,
           P(out.bytes))
    expect(out, None, want.astype(np.int8), rows)
    done(c)


@pytest.mark.parametrize("cid", lc.ids("shiftgelu_lut"))
def test_shiftgelu_lut(H, cid):
    c = begin(cid)
    rows, C = c.sizes["rows"], c.sizes["C"]
    assert lc.shiftgelu_lut_route(C) == c.kernel
    rng = np.random.default_rng(C)
    f = rng.uniform(0, 1, c.period) ** 3                          # row maxima all over the table
    f[:8] = 0
    xb = np.rint(rows8(c.period, C).astype(np.float64) * f[:, None]).astype(np.int8)
    xb[8], xb[9] = -128, 127
    s, s_out = np.float32(0.03), np.float32(0.02)
    d = np.float32(s * np.float32(2.0 ** -7))
    want = orc().requant(orc().shiftgelu(xb, s).astype(np.int32), orc().dyadic(d, s_out), 8)
    tab = torch.empty(65536, dtype=torch.int8, device="cuda")
    H.call("ivit_shiftgelu_build_table", float(s), dyv(iv.freeze.dyadic(d, s_out)), P(tab))
    x, out = rep(xb, rows), Buf(rows * C)
    H.call("ivit_shiftgelu_requant_lut", P(x), rows, C, P(tab), P(out.bytes))
    expect(out, None, want.astype(np.int8), rows)
    assert len(np.unique(xb.max(axis=1))) >= 100
    done(c)


@pytest.mark.parametrize("cid", lc.ids("shiftmax"))
def test_shiftmax(H, cid):
    c = begin(cid)
    rows, n, bits = c.sizes["rows"], c.sizes["n"], c.sizes["bits"]
    xb = sw.shiftmax_rows(n)                                      # every row maximum, flat and one-hot rows
    assert xb.shape[0] == c.period
    s = np.float32(0.1947)
    want = orc().shiftmax(xb, s, bits)
    x, out = rep(xb, rows), Buf(rows * n * 2)
    H.call("ivit_shiftmax", P(x), rows, n, n, float(s), bits, P(out.bytes), n)
    expect(out, None, want, rows)
    done(c)


@pytest.mark.parametrize("cid", lc.ids("linear_requant"))
def test_linear_requant_unplanned(H, cid):
    c = begin(cid)
    M, N, K, bits = (c.sizes[k] for k in ("M", "N", "K", "bits"))
    assert lc.linear_route(M, N, K) == c.kernel
    xb, want = linear_want(c.period, N, K, bits)
    w, b, s_pre, s_out = layer(N, K, bits)
    x, out = rep(xb, M), Buf(M * N * bits // 8)
    H.call("ivit_linear_i8_requant", P(x), P(dev(w)), P(dev(b)), P(dev(iv.freeze.dyadic(s_pre, s_out))), bits, P(out.bytes), M, N, K)
    expect(out, None, want.astype(np.int8 if bits == 8 else np.int16), M)
    done(c)


@pytest.mark.parametrize("cid", lc.ids("linear_residual"))
def test_linear_residual_unplanned(H, cid):
    c = begin(cid)
    M, N, K = (c.sizes[k] for k in ("M", "N", "K"))
    assert lc.linear_route(M, N, K) == c.kernel
    xb, resb, want = residual_want(c.period, N, K)
    w, b, s_pre, s_out = layer(N, K, 16)
    x, res, out = rep(xb, M), rep(resb, M), Buf(M * N * 2)
    H.call("ivit_linear_i8_requant_residual", P(x), P(dev(w)), P(dev(b)), P(dev(iv.freeze.dyadic(s_pre, s_out))), dyv(iv.freeze.dyadic(S_MID, S_FIN)),
           dyv(iv.freeze.dyadic(S_RES, S_FIN)), P(res), P(out.bytes), M, N, K)
    expect(out, None, want.astype(np.int16), M)
    done(c)


@pytest.mark.parametrize("cid", lc.ids("attention"))
def test_attention_fused(H, cid):
    """q.k^T -> qact_attn1 -> Shiftmax(16) -> attn.v -> qact2 (the chain of test_fused_attention_core_vs_oracle) on a block of images"""
    c = begin(cid)
    B, H_, T, dh, ldv = (c.sizes[k] for k in ("B", "H", "T", "dh", "ldv"))
    pi, o = c.period, orc()
    rng = np.random.default_rng(T)
    q, k, v = (rng.integers(-128, 128, (pi * H_, T, dh), dtype=np.int8) for _ in range(3))
    scale, s_acc = np.float32(0.1947), np.float32(2.2e-4)
    s8 = o.requant(o.bmm_nt_i8(q, k), o.dyadic(s_acc, scale), 8).astype(np.int8)
    ctx = o.bmm_av(o.shiftmax(s8, scale, 16), v)
    ref = o.requant(ctx, o.dyadic(np.float32(2.0 ** -15 * 0.1), np.float32(0.05)), 8)
    ref = ref.reshape(pi, H_, T, dh).transpose(0, 2, 1, 3).reshape(pi, T * H_ * dh).astype(np.int8)
    vt = np.zeros((pi * H_, dh, ldv), np.int8)
    vt[:, :, :T] = v.transpose(0, 2, 1)
    qd, kd, vd = rep(q.reshape(pi, -1), B), rep(k.reshape(pi, -1), B), rep(vt.reshape(pi, -1), B)
    out = Buf(B * T * H_ * dh)
    H.call("ivit_attention_fused", P(qd), P(kd), P(vd), dyv(iv.freeze.dyadic(s_acc, scale)), float(scale),
           dyv(iv.freeze.dyadic(np.float32(2.0 ** -15 * 0.1), np.float32(0.05))), P(out.bytes), B, H_, T, dh, ldv)
    expect(out, None, ref, B)
    assert len(np.unique(ref)) > 10
    done(c)


@pytest.mark.parametrize("cid", lc.ids("window_attention"))
def test_window_attention(H, cid):
    from test_swin_window12_gpu import chain_window_attention, _peaked_qkv
    c = begin(cid)
    B, R, heads, shift = (c.sizes[k] for k in ("B", "R", "heads", "shift"))
    pi, o = c.period, orc()
    rng = np.random.default_rng(1000 * R + 10 * shift + heads)
    qkv = _peaked_qkv(rng, pi, R, heads)
    relb = rng.integers(-40, 41, (heads, 49, 49)).astype(np.int16)
    s = np.float32(0.0523)
    dqk, da, dpv = o.dyadic(np.float32(0.0021), np.float32(0.047)), o.dyadic(np.float32(0.047), s), o.dyadic(np.float32(2.0 ** -7 * 0.031), np.float32(0.029))
    ref = chain_window_attention(qkv, relb, dqk, da, dpv, s, R, shift, heads, ws=7)
    qd, out = rep(qkv.reshape(pi, -1), B), Buf(B * R * R * heads * 32)
    H.call("ivit_window_attention_fused", P(qd), dyv(dqk), dyv(da), P(dev(relb)), float(s), dyv(dpv), P(out.bytes), B, R, 7, shift, heads, 32)
    expect(out, None, ref.reshape(pi, -1), B)
    assert len(np.unique(ref)) > 10
    done(c)


@pytest.mark.parametrize("cid", lc.ids("mlp_planned"))
def test_mlp_fused_planned(H, cid):
    from test_mlp192_gpu import Case as Mlp192
    c = begin(cid)
    M, C = c.sizes["M"], c.sizes["C"]
    m = Mlp192(H, c.period, seed=1000 + c.period)
    try:
        _, _, want = m.oracle(np.arange(c.period))
        x, res, out = rep(m.x, M), rep(m.res, M), Buf(M * C * 2)
        H.call("ivit_mlp_fused_planned", m.mp, P(x), P(m.tab), dyv(m.dm), dyv(m.dr), P(res), P(out.bytes), M)
        expect(out, None, want.astype(np.int16), M)
        assert len(np.unique(want)) > 10000
    finally:
        m.close()
    done(c)


@pytest.mark.parametrize("cid", lc.ids("mlp_swin"))
def test_swin_mlp_fused(H, cid):
    """the chain of test_mlp_fused_vs_oracle at C = 96, hidden = 384"""
    c = begin(cid)
    M, C, HD, p, o = c.sizes["M"], 96, 384, c.period, orc()
    rng = np.random.default_rng(p + 1)
    x = rng.integers(-128, 128, (p, C), dtype=np.int8)
    w1 = rng.integers(-128, 128, (HD, C), dtype=np.int8); b1 = rng.integers(-3000, 3000, HD).astype(np.int32)
    w2 = rng.integers(-128, 128, (C, HD), dtype=np.int8); b2 = rng.integers(-3000, 3000, C).astype(np.int32)
    s1 = (10 ** rng.uniform(-5.3, -4.9, HD)).astype(np.float32); s_h = np.float32(0.012)
    s_gelu_in, s_g = np.float32(0.03), np.float32(0.02)
    s2 = (10 ** rng.uniform(-5.6, -5.2, C)).astype(np.float32); s_t = np.float32(2e-4)
    res = rng.integers(-30000, 30000, (p, C)).astype(np.int16)
    h8 = o.requant(o.linear_i8(x, w1, b1), o.dyadic(s1, s_h), 8).astype(np.int8)
    g8 = o.requant(o.shiftgelu(h8, s_gelu_in).astype(np.int32), o.dyadic(np.float32(s_gelu_in * np.float32(2.0 ** -7)), s_g), 8).astype(np.int8)
    t = o.requant(o.linear_i8(g8, w2, b2), o.dyadic(s2, s_t), 16)
    ref = o.requant(t, o.dyadic(s_t, S_FIN), 16, res.astype(np.int32), o.dyadic(S_RES, S_FIN))
    tab = torch.empty(65536, dtype=torch.int8, device="cuda")
    H.call("ivit_shiftgelu_build_table", float(s_gelu_in), dyv(iv.freeze.dyadic(np.float32(s_gelu_in * np.float32(2.0 ** -7)), s_g)), P(tab))
    keep = [dev(a) for a in (w1, b1, iv.freeze.dyadic(s1, s_h), w2, b2, iv.freeze.dyadic(s2, s_t))]
    xd, rd, out = rep(x, M), rep(res, M), Buf(M * C * 2)
    H.call("ivit_mlp_fused", P(xd), P(keep[0]), P(keep[1]), P(keep[2]), P(tab), P(keep[3]), P(keep[4]), P(keep[5]), dyv(iv.freeze.dyadic(s_t, S_FIN)),
           dyv(iv.freeze.dyadic(S_RES, S_FIN)), P(rd), P(out.bytes), M, C, HD)
    expect(out, None, ref.astype(np.int16), M)
    done(c)


# ---------------------------------------------------------------- the 65535 of gridDim.y
def gather_patches(img, Pp):
    """the numpy gather: NCHW -> [B * gh * gw, Cin * P * P], element order (c, py, px)"""
    B, Cin, Hh, W = img.shape
    gh, gw = Hh // Pp, W // Pp
    return np.ascontiguousarray(img.reshape(B, Cin, gh, Pp, gw, Pp).transpose(0, 2, 4, 1, 3, 5)).reshape(B * gh * gw, Cin * Pp * Pp)


@pytest.mark.parametrize("cid", lc.ids("im2col"))
def test_im2col_patch(H, cid):
    c = begin(cid)
    B, Cin, HW, Pp = (c.sizes[k] for k in ("B", "Cin", "HW", "P"))
    assert lc.im2col_route(B, Cin, HW, Pp) == c.kernel
    ib = np.random.default_rng(3).integers(-128, 128, (c.period, Cin, HW, HW), dtype=np.int8)
    want = gather_patches(ib, Pp).reshape(c.period, -1)
    img, rows = rep(ib, B), Buf(B * Cin * HW * HW)
    H.call("ivit_im2col_patch", P(img), B, Cin, HW, HW, Pp, P(rows.bytes))
    expect(rows, None, want, B)
    done(c)


@functools.lru_cache(maxsize=None)
def embed_case(p, Cin, HW, D):
    """PatchEmbed on 16 x 16 patches: images, weights and the oracle's conv -> QuantAct(16) -> + pos -> QuantAct(16) of a block"""
    o, rng = orc(), np.random.default_rng(p * 131 + HW + D)
    g = HW // 16
    np_, K, T = g * g, Cin * 256, g * g + 1
    img = rng.integers(-128, 128, (p, Cin, HW, HW), dtype=np.int8)
    w = np.rint(rng.normal(0, 40, (D, K)).clip(-128, 127)).astype(np.int8)
    b = rng.integers(-2 ** 14, 2 ** 14, D).astype(np.int32)
    s_pre = (10 ** rng.uniform(-5.5, -5, D)).astype(np.float32)
    z_cls = rng.integers(-10 ** 6, 10 ** 6, D).astype(np.int32)
    pos = rng.integers(-20000, 20000, (T, D)).astype(np.int16)
    sx, sp, so = np.float32(2e-4), np.float32(5e-4), np.float32(7e-4)
    patch16 = o.requant(o.linear_i8(gather_patches(img, 16), w, b), o.dyadic(s_pre, sx), 16).reshape(p, np_, D)
    rows = np.concatenate([np.broadcast_to(z_cls, (p, 1, D)), patch16], axis=1)                       # class token's accumulators, then the patches
    x16 = o.requant(rows.reshape(p * T, D), o.dyadic(sx, so), 16, np.broadcast_to(pos.astype(np.int32), (p, T, D)).reshape(p * T, D), o.dyadic(sp, so))
    return dict(img=img, w=w, b=b, d=iv.freeze.dyadic(s_pre, sx), z_cls=z_cls, pos=pos, dx=iv.freeze.dyadic(sx, so), dp=iv.freeze.dyadic(sp, so),
                patch16=patch16.astype(np.int16), x16=x16.astype(np.int16).reshape(p, T * D), np_=np_, K=K, T=T)


@pytest.mark.parametrize("cid", lc.ids("patch_embed"))
def test_patch_embed(H, cid):
    """B = 65535: the one-launch form equals the oracle and the three-launch chain; B = 65536: refused, the output untouched"""
    c = begin(cid)
    B, Cin, HW, D = (c.sizes[k] for k in ("B", "Cin", "HW", "D"))
    e = embed_case(c.period, Cin, HW, D)
    np_, K, T = e["np_"], e["K"], e["T"]
    assert lc.patch_embed_ok(B, np_, T, D, K) == (c.side == "near")
    img, got = rep(e["img"], B), Buf(B * T * D * 2)
    w, b, d, z_cls, pos = (dev(e[k]) for k in ("w", "b", "d", "z_cls", "pos"))
    st = status(H, "ivit_patch_embed", P(img), B, Cin, HW, HW, 16, P(w), P(b), P(d), P(z_cls), P(pos), dyv(e["dx"]), dyv(e["dp"]), P(got.bytes), D)
    torch.cuda.synchronize()
    if c.side == "far":
        assert st == UNSUPPORTED, (st, err(H))
        assert got.untouched() and got.intact()
    else:
        assert st == 0, err(H)
        expect(got, None, e["x16"], B)
        rows, p16, chain = Buf(B * np_ * K), Buf(B * np_ * D * 2), Buf(B * T * D * 2)
        H.call("ivit_im2col_patch", P(img), B, Cin, HW, HW, 16, P(rows.bytes))
        H.call("ivit_linear_i8_requant", P(rows.bytes), P(w), P(b), P(d), 16, P(p16.bytes), B * np_, D, K)
        H.call("ivit_embed_finish", P(p16.bytes), P(z_cls), P(pos), dyv(e["dx"]), dyv(e["dp"]), P(chain.bytes), B, T, D)
        torch.cuda.synchronize()
        assert torch.equal(got.bytes, chain.bytes) and rows.intact() and p16.intact() and chain.intact()
    done(c, f"status {st}")


@pytest.mark.parametrize("cid", lc.ids("embed_finish"))
def test_embed_finish(H, cid):
    c = begin(cid)
    B, T, D = (c.sizes[k] for k in ("B", "T", "D"))
    e = embed_case(c.period, 3, 16, D)
    assert e["T"] == T and lc.embed_finish_ok(B, T, D) == (c.side == "near")
    p16, got = rep(e["patch16"].reshape(c.period, -1), B), Buf(B * T * D * 2)
    st = status(H, "ivit_embed_finish", P(p16), P(dev(e["z_cls"])), P(dev(e["pos"])), dyv(e["dx"]), dyv(e["dp"]), P(got.bytes), B, T, D)
    torch.cuda.synchronize()
    if c.side == "far":
        assert st == INVALID and "2^16" in err(H), (st, err(H))
        assert got.untouched() and got.intact()
    else:
        assert st == 0, err(H)
        expect(got, None, e["x16"], B)
    done(c, f"status {st}")


@pytest.mark.parametrize("cid", lc.ids("attn_qk"))
def test_attn_qk_batch(H, cid):
    """the batched products take one matrix per gridDim.y: 65535 of them run, 65536 are refused before the launch"""
    c = begin(cid)
    BH, T, dh, lds = (c.sizes[k] for k in ("BH", "T", "dh", "lds"))
    assert lc.batched_ok(BH) == (c.side == "near")
    o, rng = orc(), np.random.default_rng(11)
    q, k = (rng.integers(-128, 128, (c.period, T, dh), dtype=np.int8) for _ in range(2))
    s_acc, s = np.float32(4.0e-4), np.float32(0.05)
    want = np.full((c.period, T, lds), FILL8, np.int8)            # the columns j >= T of a row are not written
    want[:, :, :T] = o.requant(o.bmm_nt_i8(q, k), o.dyadic(s_acc, s), 8)
    qd, kd, out = rep(q.reshape(c.period, -1), BH), rep(k.reshape(c.period, -1), BH), Buf(BH * T * lds)
    st = status(H, "ivit_attn_qk_requant", P(qd), P(kd), dyv(iv.freeze.dyadic(s_acc, s)), P(out.bytes), BH, T, dh, lds)
    torch.cuda.synchronize()
    if c.side == "far":
        assert st == UNSUPPORTED and "65535" in err(H), (st, err(H))
        assert out.untouched() and out.intact()
    else:
        assert st == 0, err(H)
        expect(out, None, want.reshape(c.period, -1), BH)
        assert len(np.unique(want)) > 50
    done(c, f"status {st}")


# ---------------------------------------------------------------- a launch holds fewer than 2^32 work-items
@pytest.mark.parametrize("cid", lc.ids("shiftmax_limit"))
def test_shiftmax_work_items(H, cid):
    """(2^24 - 1) * 4 rows are 2^24 - 1 blocks of 256 threads and run; one row more is 2^32 work-items: refused, nothing written"""
    c = begin(cid)
    rows, n, bits = c.sizes["rows"], c.sizes["n"], c.sizes["bits"]
    assert lc.launch_fits((rows + 3) // 4, 256) == (c.side == "near")
    xb = sw.shiftmax_rows(n)
    s = np.float32(0.1947)
    want = orc().shiftmax(xb, s, bits)
    x, out = rep(xb, rows), Buf(rows * n * 2)
    st = status(H, "ivit_shiftmax", P(x), rows, n, n, float(s), bits, P(out.bytes), n)
    torch.cuda.synchronize()
    if c.side == "far":
        assert st == UNSUPPORTED and "2^32 work-items" in err(H) and str(rows - 1) in err(H), (st, err(H))
        assert out.untouched() and out.intact()
    else:
        assert st == 0, err(H)
        expect(out, None, want, rows)
    done(c, f"status {st}")


@pytest.mark.parametrize("cid", lc.ids("layernorm_limit"))
def test_layernorm_work_items(H, cid):
    """ivit_layernorm at its narrowest width, 8 rows per block: (2^24 - 1) * 8 rows run, one more is refused"""
    c = begin(cid)
    rows, C = c.sizes["rows"], c.sizes["C"]
    assert lc.launch_fits((rows + 7) // 8, 256) == (c.side == "near")
    xb = tokens16(c.period, C)[0]
    bias_int, sc = norm_consts(C)
    want = orc().layernorm(xb, float(S_IN), bias_int, sc)
    x, out = rep(xb, rows), Buf(rows * C * 4)
    st = status(H, "ivit_layernorm", P(x), rows, C, float(S_IN), P(dev(bias_int)), P(dev(sc)), P(out.bytes))
    torch.cuda.synchronize()
    if c.side == "far":
        assert st == UNSUPPORTED and "2^32 work-items" in err(H) and str(rows - 1) in err(H), (st, err(H))
        assert out.untouched() and out.intact()
    else:
        assert st == 0, err(H)
        expect(out, None, want, rows)
    done(c, f"status {st}")


@pytest.mark.parametrize("cid", lc.ids("topk_limit"))
def test_logits_topk_work_items(H, cid):
    """one wavefront per image, four per block: 2^26 - 3 images are 2^32 work-items, refused with idx and val untouched"""
    c = begin(cid)
    batch, ncls, k = c.sizes["batch"], c.sizes["ncls"], c.sizes["k"]
    assert not lc.launch_fits((batch + 3) // 4, 256) and lc.launch_fits((batch + 2) // 4, 256)
    logits = torch.zeros(batch, ncls, dtype=torch.int32, device="cuda")
    idx, val = Buf(batch * k * 4), Buf(batch * k * 4)
    st = status(H, "ivit_logits_topk", P(logits), P(dev(np.ones(ncls, np.float32))), batch, ncls, k, P(idx.bytes), P(val.bytes))
    torch.cuda.synchronize()
    assert st == UNSUPPORTED and "2^32 work-items" in err(H) and str(batch - 1) in err(H), (st, err(H))
    assert idx.untouched() and val.untouched() and idx.intact() and val.intact()
    done(c, f"status {st}")


@pytest.mark.parametrize("cid", lc.ids("hidden_f32"))
def test_hidden_f32(H, cid):
    from ivit_amd.predict import hidden_reference
    c = begin(cid)
    batch, T, C, t0, layout = (c.sizes[k] for k in ("batch", "T", "C", "t0", "layout"))
    qb = rows16(c.period, T * C).reshape(c.period, T, C)
    scale = np.float32(3.1e-4)
    want = hidden_reference(qb, scale, layout, t0)
    x, out = rep(qb.reshape(c.period, -1), batch), Buf(batch * (T - t0) * C * 4)
    H.call("ivit_hidden_f32", P(x), float(scale), batch, T, C, t0, _lib.IVIT_HIDDEN_GRID if layout == "grid" else _lib.IVIT_HIDDEN_TOKENS, P(out.bytes))
    expect(out, None, want.reshape(c.period, -1), batch)
    done(c)


# ---------------------------------------------------------------- the ViT runner
@pytest.fixture(scope="module")
def engines():
    """the engines of the runner cases, built once each; they hold their workspaces and are released with the module"""
    made = {}
    yield made
    made.clear()


def runner_engine(_ENGINES, model):
    """(cfg, engine, block of images, the oracle's logits of the block): micro_vit on its golden scales (patch 8: im2col -> GEMM ->
    embed_finish), or a self-calibrated config with 16 x 16 patches (one PatchEmbed launch), built as
    test_random_shapes_self_calibrated_engine_vs_oracle builds its configs"""
    if model not in _ENGINES:
        if model == "micro_vit":
            from ivit_amd.engine import ViTEngine
            g = load_golden("micro_vit_b2.npz")
            cfg = iv.CONFIGS[str(g["cfg_name"])]
            w, scales = iv.make_vit_weights(cfg, int(g["seed"])), golden_scales(g)
            eng = ViTEngine.from_float(cfg, w, scales)
        else:
            s = lc.RUNNER_MODELS[model]
            cfg = iv.ViTConfig("large_" + model, img_size=s["img"], patch_size=s["patch"], num_classes=s["ncls"], embed_dim=s["D"], depth=s["depth"],
                               num_heads=s["heads"])
            w = iv.make_vit_weights(cfg, seed=len(model) + s["D"])
            m = iv.VisionTransformer(img_size=s["img"], patch_size=s["patch"], num_classes=s["ncls"], embed_dim=s["D"], depth=s["depth"],
                                     num_heads=s["heads"], mlp_ratio=4)
            m.load_float_weights(w)
            with torch.no_grad():
                m(dev(iv.make_calibration_batch(cfg, 3, seed=17)))
            iv.freeze_model(m)
            scales = {k: v for k, v in m.act_scales().items() if v > 0}
            eng = m.compile()
        block = iv.make_images_int8(cfg, 7, seed=4)
        ref, _ = orc().OracleViT(cfg, w, scales).forward(block)
        _ENGINES[model] = (cfg, eng, block, ref.astype(np.int32))
    return _ENGINES[model]


@pytest.mark.parametrize("cid", lc.ids("runner"))
def test_vit_runner_slice_limit(engines, cid):
    """the largest slice a model takes (65535 images; 65535 / heads without the fused attention): the forward equals forwards in
    chunks of 4096 and the oracle; one image more in one slice: refused before anything is launched, the limit named in the runner's own
    terms; the same batch in two slices: correct"""
    c = begin(cid)
    model, batch, nslices = c.sizes["model"], c.sizes["batch"], c.sizes["nslices"]
    cfg, eng, block, ref = runner_engine(engines, model)
    limit = c.sizes["limit"]
    assert lc.max_slice_images(cfg.head_dim == 64 and cfg.num_tokens <= 640, cfg.num_heads) == limit
    need = ctypes.c_size_t()
    eng._entry("_workspace_bytes", eng.model, batch, nslices, ctypes.byref(need))
    assert need.value <= c.arrays["workspace"], (need.value, c.arrays["workspace"])
    imgs = rep(block.reshape(7, -1), batch).view(batch, *block.shape[1:])
    if c.kernel == "IVIT_ERR_UNSUPPORTED":
        with pytest.raises(_lib.IvitError, match=rf"unsupported shape.*{limit + 1} images per slice.*at most {limit} per slice") as ei:
            eng.forward(imgs, nslices=nslices)
        assert "ivit_embed_finish" not in str(ei.value) and "ivit_attn_qk" not in str(ei.value) and "ivit_vit_forward" in str(ei.value)
    else:
        got = eng.forward(imgs, nslices=nslices).clone()
        torch.cuda.synchronize()
        row = lc.first_mismatch(torch, got, dev(ref))
        assert row is None, f"first differing image {row}"
        if nslices == 1:
            for b0 in range(0, batch, 4096):
                assert torch.equal(eng.forward(imgs[b0:b0 + 4096].contiguous()), got[b0:b0 + 4096]), b0
    done(c)
