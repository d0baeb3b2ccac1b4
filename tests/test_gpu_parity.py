"""GPU parity: HIP path (through the C-ABI) vs reference golden vectors and the CPU oracle.
Bit-exact everywhere (integer outputs)."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden, golden_scales

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from abi_cases import ln_lds_case as _ln_lds_case  # noqa: E402

_P = ctypes.c_void_p


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


_KEEP = []


def dev(a):
    """host -> device; the tensor is kept alive (raw pointers are handed to the C-ABI)."""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    _KEEP.append(t)
    if len(_KEEP) > 64:
        torch.cuda.synchronize()
        del _KEEP[:32]
    return t


def P(t):
    return _P(t.data_ptr())


def dy_dev(s_pre, s_out):
    d = iv.freeze.dyadic(s_pre, s_out)
    return d, dev(d)


def dyv(d):
    return _lib.Dyadic(float(d[0, 0]), float(d[0, 1]))


def test_library_loaded():
    lib = _lib.load()
    assert lib.ivit_version() >= 100


def test_lean_division(H):
    """hoisted-reciprocal division == IEEE division, bit for bit, on the path's value ranges:
    requotient (Q*s)/s, shift-exp t/x0, LayerNorm (o*sc)/sc."""
    rng = np.random.default_rng(5)
    cases = []
    for s in (10 ** rng.uniform(-6, 0.5, 400)).astype(np.float32):      # (Q*s)/s, all int16 Q
        q = np.arange(-32768, 32768, 1, dtype=np.float32)[rng.integers(0, 65536, 4096)]
        cases.append(((q * s).astype(np.float32), np.full(4096, s, np.float32)))
    for x0 in -rng.integers(1, 4000, 300).astype(np.float32):             # t / x0
        t = -(rng.uniform(0, 400, 4096)).astype(np.float32)
        cases.append((t, np.full(4096, x0, np.float32)))
    for _ in range(300):                                                   # (o*sc)/sc, o ~ 2^28
        sc = np.float32(rng.uniform(-1, 1) * 3e-5)
        o = np.rint(rng.standard_normal(4096) * 2 ** 28).astype(np.float32)
        cases.append(((o * sc).astype(np.float32), np.full(4096, sc, np.float32)))
    n = np.concatenate([c[0] for c in cases])
    d = np.concatenate([c[1] for c in cases])
    nd, dd = dev(n), dev(d)
    a = torch.empty_like(nd)
    b = torch.empty_like(nd)
    H.call("ivit_debug_div", P(nd), P(dd), P(a), P(b), n.size)
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.array_equal(a, (n / d).astype(np.float32))     # GPU IEEE division == host IEEE
    assert np.array_equal(a.view(np.int32), b.view(np.int32)), f"{(a != b).sum()} of {n.size} differ"


def test_markstein_requotient(H):
    """fl(fl(q*d)/d) by product + exact residual + one correction with RN(1/d) (ivit_layernorm.h::requotient_m) equals
    the IEEE sequence bit for bit: every int16 Q against many per-tensor scales (quant_modules.py:204-206 -> :359), and
    24-bit |o| up to 2^31 against per-channel LayerNorm scales of either sign (quant_modules.py:378-386 -> quant_utils.py:220)."""
    rng = np.random.default_rng(11)
    qs, ds = [], []
    allq = np.arange(-32768, 32768, dtype=np.float32)
    for s in (10 ** rng.uniform(-6, 0.5, 48)).astype(np.float32):
        qs.append(allq)
        ds.append(np.full(allq.size, s, np.float32))
    for _ in range(600):
        sc = np.float32(rng.uniform(-1, 1) * 10 ** rng.uniform(-9, -3))
        if sc == 0:
            continue
        o = np.rint(rng.standard_normal(4096) * 2.0 ** rng.integers(8, 31)).astype(np.float32) + np.float32(0)   # no -0.0
        qs.append(o)
        ds.append(np.full(4096, sc, np.float32))
    q = np.concatenate(qs)
    d = np.concatenate(ds)
    a = torch.empty(q.size, dtype=torch.float32, device="cuda")
    b = torch.empty_like(a)
    H.call("ivit_debug_requotient", P(dev(q)), P(dev(d)), P(a), P(b), q.size)
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.array_equal(a, ((q * d).astype(np.float32) / d).astype(np.float32))     # GPU IEEE == host IEEE
    assert np.array_equal(a.view(np.int32), b.view(np.int32)), f"{(a != b).sum()} of {q.size} differ"


def test_quantize_input(H, ops_golden):
    g = ops_golden
    x = dev(g["quant_in/x"])
    q = torch.empty(x.shape, dtype=torch.int8, device="cuda")
    H.call("ivit_quantize_input_f32", P(x), float(g["quant_in/s"]), P(q), x.numel())
    assert np.array_equal(q.cpu().numpy(), g["quant_in/out"])


def test_shiftmax_golden(H, ops_golden):
    g = ops_golden
    for i in range(int(g["shiftmax/n"])):
        x = g[f"shiftmax/{i}/x"]
        rows, n = x.shape
        ld = (n + 15) // 16 * 16
        xp = np.zeros((rows, ld), np.int8)
        xp[:, :n] = x
        out = torch.zeros(rows, ld, dtype=torch.int16, device="cuda")
        H.call("ivit_shiftmax", P(dev(xp)), rows, n, ld, float(g[f"shiftmax/{i}/s"]),
               int(g[f"shiftmax/{i}/bits"]), P(out), ld)
        got = out.cpu().numpy().view(np.uint16)[:, :n]
        assert np.array_equal(got, g[f"shiftmax/{i}/out"]), i


def test_shiftgelu_golden(H, ops_golden):
    g = ops_golden
    for i in range(int(g["gelu/n"])):
        x = g[f"gelu/{i}/x"]
        rows, C = x.shape
        out = torch.empty(rows, C, dtype=torch.int16, device="cuda")
        H.call("ivit_shiftgelu", P(dev(x)), rows, C, float(g[f"gelu/{i}/s"]), P(out))
        assert np.array_equal(out.cpu().numpy(), g[f"gelu/{i}/out"]), i


def test_shiftgelu_lut_equals_direct(H, ops_golden):
    """table form == direct fp32-faithful form == reference golden (after requant)."""
    g = ops_golden
    from oracle import oracle as orc
    for i in range(int(g["gelu/n"])):
        x = g[f"gelu/{i}/x"]
        rows, C = x.shape
        s = float(g[f"gelu/{i}/s"])
        d = iv.freeze.dyadic(np.float32(np.float32(s) * np.float32(2.0 ** -7)), np.float32(0.0143))
        xd = dev(x)
        direct = torch.empty(rows, C, dtype=torch.int8, device="cuda")
        H.call("ivit_shiftgelu_requant", P(xd), rows, C, s, dyv(d), P(direct))
        tab = torch.empty(65536, dtype=torch.int8, device="cuda")
        H.call("ivit_shiftgelu_build_table", s, dyv(d), P(tab))
        lut = torch.empty(rows, C, dtype=torch.int8, device="cuda")
        H.call("ivit_shiftgelu_requant_lut", P(xd), rows, C, P(tab), P(lut))
        ref = orc.requant(g[f"gelu/{i}/out"].astype(np.int32), orc.dyadic(np.float32(np.float32(s) * np.float32(2.0 ** -7)), np.float32(0.0143)), 8)
        assert np.array_equal(direct.cpu().numpy().astype(np.int32), ref), i
        assert np.array_equal(lut.cpu().numpy(), direct.cpu().numpy()), i


def test_layernorm_golden(H, ops_golden):
    g = ops_golden
    for i in range(int(g["ln/n"])):
        x = g[f"ln/{i}/x"]
        rows, C = x.shape
        bias_int, sc = iv.freeze.layernorm_constants(g[f"ln/{i}/w"], g[f"ln/{i}/b"])
        z = torch.empty(rows, C, dtype=torch.float32, device="cuda")
        H.call("ivit_layernorm", P(dev(x)), rows, C, float(g[f"ln/{i}/s"]), P(dev(bias_int)), P(dev(sc)), P(z))
        assert np.array_equal(z.cpu().numpy(), g[f"ln/{i}/z"]), i
        d, dd = dy_dev(sc, g[f"ln/{i}/s_out"])
        o8 = torch.empty(rows, C, dtype=torch.int8, device="cuda")
        H.call("ivit_layernorm_requant", P(dev(x)), rows, C, C, float(g[f"ln/{i}/s"]), P(dev(bias_int)),
               P(dev(sc)), P(dd), P(o8))
        assert np.array_equal(o8.cpu().numpy(), g[f"ln/{i}/out8"]), i


@pytest.mark.parametrize("C", [384, 768, 192, 1024])
def test_layernorm_requant_vs_oracle_ragged(H, C):
    """I-LayerNorm + per-channel QuantAct(8) against the CPU oracle (quant_modules.py:353-386, quant_utils.py:213-253) on
    random rows at four channel counts (S = 2 and S = 4 lane splits of layernorm_reg_kernel): row counts that leave dead lane
    groups in the last wave and the last block, a strided input (the class-token rows of the final norm), scales with both
    signs, a guard row behind the output.  (Round 6 wrote it for the hand-packed variant of the kernel, which was measured and
    not kept — tools/experiments/ivit_layernorm_pk.h; the shipped kernel had no oracle test on ragged random rows either.)"""
    from oracle import oracle as orc
    rng = np.random.default_rng(C)
    w = rng.normal(1.0, 0.4, C).astype(np.float32) * rng.choice([-1.0, 1.0], C).astype(np.float32)
    b = rng.normal(0.0, 0.5, C).astype(np.float32)
    bias_int, sc = iv.freeze.layernorm_constants(w, b)
    s_in, s_out = np.float32(7.3e-4), np.float32(0.031)
    d, dd = dy_dev(sc, s_out)
    for rows, stride in ((1, C), (7, C), (33, C), (1000, C), (4099, C), (64, 3 * C)):
        x = rng.integers(-26000, 26000, (rows, stride // C, C)).astype(np.int16)
        x[:, 0, : C // 2] //= 64                                      # small and large magnitudes in one row
        want = orc.requant(orc.layernorm(np.ascontiguousarray(x[:, 0]), float(s_in), bias_int, sc), orc.dyadic(sc, s_out), 8)
        o8 = torch.full((rows + 1, C), 77, dtype=torch.int8, device="cuda")
        H.call("ivit_layernorm_requant", P(dev(x)), rows, C, stride, float(s_in), P(dev(bias_int)), P(dev(sc)), P(dd), P(o8))
        got = o8.cpu().numpy()
        assert np.array_equal(got[:rows].astype(np.int32), want), (C, rows, stride, int((got[:rows] != want).sum()))
        assert (got[rows] == 77).all()
        assert len(np.unique(want)) > 50


@pytest.mark.parametrize("device", [0, 1])
def test_layernorm_dynamic_lds_attribute_cache(device):
    """The dynamic-LDS attribute of a kernel is set once per device and kernel for the largest size seen (launch_dyn, ivit_hip.hip).
    ivit_layernorm on 8 rows launches layernorm_kernel<false> with 8 * C * 4 bytes of LDS: C = 2056 (65 792 B, the first size above
    64 KB: the attribute is set), 4096 (131 072 B: the request grows, set again), 2056 again (below the cached maximum: no host call,
    and the launch must still be accepted), 512 (below 64 KB: the cache is not consulted).  Each result equals the oracle's bit for
    bit.  Device 1 (after device 0, in the same process) repeats the first two steps: its cache entry is its own."""
    if device >= torch.cuda.device_count():
        pytest.skip("one visible GPU: the second-device half of the per-device attribute cache is not exercised")
    with torch.cuda.device(device):
        Hd = _lib.Handle(device, torch.cuda.current_stream().cuda_stream)
        for C in (2056, 4096, 2056, 512) if device == 0 else (2056, 4096):
            x, bias_int, sc, want = _ln_lds_case(C)
            z = torch.zeros(8, C, dtype=torch.float32, device="cuda")
            Hd.call("ivit_layernorm", P(dev(x)), 8, C, 7.3e-4, P(dev(bias_int)), P(dev(sc)), P(z))
            got = z.cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (device, C, int((got != want).sum()))
        Hd.close()


@pytest.mark.parametrize("C,R,B", [(96, 56, 3), (192, 28, 5), (384, 14, 9), (128, 8, 2)])
def test_patch_merge_layernorm_equals_gather_then_layernorm(H, C, R, B):
    """PatchMerging's 2 x 2 gather folded into the loads of the I-LayerNorm + QuantAct(8) that follows it (swin_quant.py:336-349,
    round 6) == ivit_patch_merge_gather followed by ivit_layernorm_requant, and == the CPU oracle on the numpy gather."""
    from oracle import oracle as orc
    rng = np.random.default_rng(C + R)
    x = rng.integers(-24000, 24000, (B, R, R, C)).astype(np.int16)
    C4 = 4 * C
    w = rng.normal(1.0, 0.3, C4).astype(np.float32); b = rng.normal(0.0, 0.4, C4).astype(np.float32)
    bias_int, sc = iv.freeze.layernorm_constants(w, b)
    s_in, s_out = np.float32(6.1e-4), np.float32(0.028)
    d, dd = dy_dev(sc, s_out)
    rows = B * (R // 2) ** 2
    xd = dev(x)
    t16 = torch.empty(rows, C4, dtype=torch.int16, device="cuda")
    H.call("ivit_patch_merge_gather", P(xd), 16, B, R, C, P(t16))
    want = torch.empty(rows, C4, dtype=torch.int8, device="cuda")
    H.call("ivit_layernorm_requant", P(t16), rows, C4, C4, float(s_in), P(dev(bias_int)), P(dev(sc)), P(dd), P(want))
    got = torch.full((rows + 1, C4), 55, dtype=torch.int8, device="cuda")
    H.call("ivit_patch_merge_layernorm_requant", P(xd), B, R, C, float(s_in), P(dev(bias_int)), P(dev(sc)), P(dd), P(got))
    assert torch.equal(got[:rows], want)
    assert (got[rows] == 55).all()
    xm = np.concatenate([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], axis=-1).reshape(rows, C4)
    assert np.array_equal(t16.cpu().numpy(), xm)
    ref = orc.requant(orc.layernorm(np.ascontiguousarray(xm), float(s_in), bias_int, sc), orc.dyadic(sc, s_out), 8)
    assert np.array_equal(got[:rows].cpu().numpy().astype(np.int32), ref)
    with pytest.raises(_lib.IvitError):
        H.call("ivit_patch_merge_layernorm_requant", P(xd), B, R, 40, float(s_in), P(dev(bias_int)), P(dev(sc)), P(dd), P(got))


def test_requant_golden(H, ops_golden):
    g = ops_golden
    for i in range(int(g["requant/n"])):
        z = g[f"requant/{i}/z"]
        rows, C = z.shape
        bits = int(g[f"requant/{i}/bits"])
        d, dd = dy_dev(g[f"requant/{i}/s_pre"], g[f"requant/{i}/s_out"])
        out = torch.empty(rows, C, dtype={8: torch.int8, 16: torch.int16}[bits], device="cuda")
        if f"requant/{i}/z_id" in g.files:
            di, ddi = dy_dev(g[f"requant/{i}/s_id"], g[f"requant/{i}/s_out"])
            H.call("ivit_requant_f32", P(dev(z)), P(dd), d.shape[0], P(dev(g[f"requant/{i}/z_id"])), P(ddi),
                   bits, P(out), rows, C)
        else:
            H.call("ivit_requant_f32", P(dev(z)), P(dd), d.shape[0], None, None, bits, P(out), rows, C)
        assert np.array_equal(out.cpu().numpy().astype(np.int32), g[f"requant/{i}/out"]), i


@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (197, 192, 192), (394, 1152, 384), (50, 1000, 384),
                                   (1, 10, 64), (300, 96, 1536), (129, 130, 48)])
def test_linear_i8_vs_numpy(H, M, N, K):
    rng = np.random.default_rng(M * 7 + N)
    x = rng.integers(-128, 128, (M, K), dtype=np.int8)
    w = rng.integers(-128, 128, (N, K), dtype=np.int8)
    b = rng.integers(-2 ** 20, 2 ** 20, N).astype(np.int32)
    acc = torch.empty(M, N, dtype=torch.int32, device="cuda")
    H.call("ivit_linear_i8", P(dev(x)), P(dev(w)), P(dev(b)), P(acc), M, N, K)
    ref = x.astype(np.int32) @ w.astype(np.int32).T + b
    assert np.array_equal(acc.cpu().numpy(), ref)


@pytest.mark.parametrize("M,N,K", [(256, 128, 64), (788, 384, 384), (300, 1152, 192), (197, 1000, 384),
                                   (50, 10, 64), (513, 136, 1536), (394, 384, 48), (300, 288, 96), (257, 96, 96),
                                   (130, 384, 160), (640, 96, 352),
                                   # round 5: M >= 8192 with K = 96 / 128 / 192 runs the weights-in-registers streaming kernel
                                   # (ivit_gemm_wreg.h): channel groups of 3 and of 2 tiles, ragged last row tile
                                   (8192 + 77, 288, 96), (8300, 96, 96), (8200, 576, 192), (8193, 192, 192), (8200, 768, 192),
                                   (8250, 128, 128), (8200, 384, 128), (9000, 64, 96)])
def test_linear_requant_epilogues_vs_oracle(H, M, N, K):
    """a1+a3 fused epilogues (8-bit, 16-bit, 16-bit + residual) == oracle linear + requant.
    K % 32 == 0 (K >= 64) shapes take the global_load_lds kernel — K % 64 == 32 through its masked 32-wide
    tail step (Swin stage 0, K = 96) — and K = 48 the generic kernel."""
    from oracle import oracle as orc
    rng = np.random.default_rng(M + N + K)
    x = rng.integers(-128, 128, (M, K), dtype=np.int8)
    w = rng.integers(-128, 128, (N, K), dtype=np.int8)
    b = rng.integers(-2 ** 16, 2 ** 16, N).astype(np.int32)
    acc = orc.linear_i8(x, w, b)
    amax = float(np.abs(acc).max())
    s_pre = (10 ** rng.uniform(-6, -4, N)).astype(np.float32)
    s_pre[::5] *= 0.5
    xd, wd, bd = dev(x), dev(w), dev(b)
    for bits in (8, 16):
        s_out = np.float32(amax * float(s_pre.mean()) / 2 ** (bits - 1) * 2.0)
        d = iv.freeze.dyadic(s_pre, s_out)
        out = torch.empty(M, N, dtype={8: torch.int8, 16: torch.int16}[bits], device="cuda")
        H.call("ivit_linear_i8_requant", P(xd), P(wd), P(bd), P(dev(d)), bits, P(out), M, N, K)
        ref = orc.requant(acc, orc.dyadic(s_pre, s_out), bits)
        assert np.array_equal(out.cpu().numpy().astype(np.int32), ref), (bits, M, N, K)
    # residual form; exact-tie multipliers (ratio 0.5 / 1.5) exercise the fp64 fallback
    res = rng.integers(-32768, 32768, (M, N)).astype(np.int16)
    for s_mid, s_res, s_fin in [(3.1e-5, 7.7e-5, 9.1e-5), (1e-4, 3e-4, 2e-4)]:
        d_ch = iv.freeze.dyadic(s_pre, np.float32(amax * float(s_pre.mean()) / 32768 * 2.0))
        d_main = iv.freeze.dyadic(np.float32(s_mid), np.float32(s_fin))
        d_res = iv.freeze.dyadic(np.float32(s_res), np.float32(s_fin))
        out = torch.empty(M, N, dtype=torch.int16, device="cuda")
        H.call("ivit_linear_i8_requant_residual", P(xd), P(wd), P(bd), P(dev(d_ch)), dyv(d_main), dyv(d_res),
               P(dev(res)), P(out), M, N, K)
        t = orc.requant(acc, orc.dyadic(s_pre, np.float32(amax * float(s_pre.mean()) / 32768 * 2.0)), 16)
        ref = orc.requant(t, orc.dyadic(np.float32(s_mid), np.float32(s_fin)), 16, res.astype(np.int32),
                          orc.dyadic(np.float32(s_res), np.float32(s_fin)))
        assert np.array_equal(out.cpu().numpy().astype(np.int32), ref), (M, N, K, s_mid)


@pytest.mark.parametrize("M,N,K", [(1000, 192, 384), (777, 384, 768), (130, 768, 1536), (9000, 192, 384), (257, 100, 64)])
def test_linear_requant8_store16_vs_oracle(H, M, N, K):
    """PatchMerging's reduction -> qact2 (swin_quant.py:343-349) with the 8-bit QuantAct stored as the 16-bit stream of the next stage
    (ivit_linear_i8_requant8_store16: the EPI_RQ8W16_CH flavour of gemm_glds_kernel) == the oracle's linear + 8-bit requant, and ==
    ivit_linear_i8_requant(bits = 8) + ivit_widen_i8_i16; multipliers chosen so that a good share of the outputs saturate at -128 / 127;
    no bias like the reference's layer, and with one; guard row; a short-K shape (the streaming kernel's) is refused."""
    from oracle import oracle as orc
    rng = np.random.default_rng(M * 3 + N + K)
    x = rng.integers(-128, 128, (M, K), dtype=np.int8)
    w = rng.integers(-128, 128, (N, K), dtype=np.int8)
    xd, wd = dev(x), dev(w)
    for with_bias in (False, True):
        b = rng.integers(-2 ** 16, 2 ** 16, N).astype(np.int32) if with_bias else None
        acc = orc.linear_i8(x, w, b if with_bias else np.zeros(N, np.int32))
        s_pre = (10 ** rng.uniform(-6, -4, N)).astype(np.float32)
        s_out = np.float32(float(np.abs(acc).std()) * float(s_pre.mean()) / 128 * 1.5)        # ~ 1.5 sigma at full scale: both rails are hit
        d = iv.freeze.dyadic(s_pre, s_out)
        ref = orc.requant(acc, orc.dyadic(s_pre, s_out), 8)
        out = torch.full((M + 1, N), 0x5555, dtype=torch.int16, device="cuda")
        bd = dev(b) if with_bias else None
        H.call("ivit_linear_i8_requant8_store16", P(xd), P(wd), P(bd) if with_bias else None, P(dev(d)), P(out), M, N, K)
        assert np.array_equal(out[:M].cpu().numpy().astype(np.int32), ref), (M, N, K, with_bias)
        assert (out[M] == 0x5555).all()
        sat = float(((ref == 127) | (ref == -128)).mean())
        assert 0.02 < sat < 0.6 and len(np.unique(ref)) > 200, sat
        o8 = torch.empty(M, N, dtype=torch.int8, device="cuda")
        o16 = torch.empty(M, N, dtype=torch.int16, device="cuda")
        H.call("ivit_linear_i8_requant", P(xd), P(wd), P(bd) if with_bias else None, P(dev(d)), 8, P(o8), M, N, K)
        H.call("ivit_widen_i8_i16", P(o8), P(o16), M * N)
        assert torch.equal(out[:M], o16)
    with pytest.raises(_lib.IvitError, match="gemm_glds"):
        big = torch.zeros(8192, 96, dtype=torch.int8, device="cuda")
        H.call("ivit_linear_i8_requant8_store16", P(big), P(dev(rng.integers(-128, 128, (96, 96), dtype=np.int8))), None, P(dev(iv.freeze.dyadic(s_pre[:96].copy(), s_out))),
               P(torch.empty(8192, 96, dtype=torch.int16, device="cuda")), 8192, 96, 96)


@pytest.mark.parametrize("M,N,K", [(300, 288, 96), (8300, 288, 96), (8200, 192, 192)])
def test_linear_requant_saturating_multipliers(H, M, N, K):
    """multipliers far outside the magic-number range (|z c| >= 2^31 possible): every kernel of the QuantLinear family must
    take its v_rndne_f64 / saturating-convert path and still clamp like the reference (quant_utils.py:247-251)"""
    from oracle import oracle as orc
    rng = np.random.default_rng(N + K)
    x = rng.integers(-128, 128, (M, K), dtype=np.int8)
    w = rng.integers(-128, 128, (N, K), dtype=np.int8)
    b = rng.integers(-2 ** 16, 2 ** 16, N).astype(np.int32)
    acc = orc.linear_i8(x, w, b)
    s_pre = (10 ** rng.uniform(-3, -2, N)).astype(np.float32)
    s_pre[::7] = np.float32(3e-9)                      # a few channels stay in range: mixed group
    xd, wd, bd = dev(x), dev(w), dev(b)
    for bits in (8, 16):
        d = iv.freeze.dyadic(s_pre, np.float32(2e-7))
        out = torch.empty(M, N, dtype={8: torch.int8, 16: torch.int16}[bits], device="cuda")
        H.call("ivit_linear_i8_requant", P(xd), P(wd), P(bd), P(dev(d)), bits, P(out), M, N, K)
        ref = orc.requant(acc, orc.dyadic(s_pre, np.float32(2e-7)), bits)
        assert np.array_equal(out.cpu().numpy().astype(np.int32), ref), (bits, M, N, K)


def test_mfma_operand_order_asymmetric(H):
    """A = I (padded) against an asymmetric B catches a transposed C write."""
    K = 64
    x = np.zeros((64, K), np.int8)
    x[np.arange(64), np.arange(64)] = 1
    w = (np.arange(96 * K).reshape(96, K) % 97 - 48).astype(np.int8)
    acc = torch.empty(64, 96, dtype=torch.int32, device="cuda")
    H.call("ivit_linear_i8", P(dev(x)), P(dev(w)), None, P(acc), 64, 96, K)
    assert np.array_equal(acc.cpu().numpy(), w.astype(np.int32).T[:64])


@pytest.mark.parametrize("nb,M,N,K", [(3, 197, 197, 64), (2, 17, 17, 64), (5, 49, 49, 32)])
def test_bmm_nt_i8(H, nb, M, N, K):
    rng = np.random.default_rng(nb + M)
    A = rng.integers(-128, 128, (nb, M, K), dtype=np.int8)
    B = rng.integers(-128, 128, (nb, N, K), dtype=np.int8)
    C = torch.empty(nb, M, N, dtype=torch.int32, device="cuda")
    H.call("ivit_bmm_nt_i8", P(dev(A)), P(dev(B)), P(C), nb, M, N, K, K, K, N, M * K, N * K, M * N)
    ref = np.einsum("bmk,bnk->bmn", A.astype(np.int32), B.astype(np.int32))
    assert np.array_equal(C.cpu().numpy(), ref)


@pytest.mark.parametrize("nb,M,N,K", [(3, 197, 64, 197), (2, 17, 64, 17), (2, 130, 32, 577)])
def test_bmm_nt_u16i8_full_range(H, nb, M, N, K):
    """16-bit probabilities incl. the extreme values 0, 32640..32768."""
    rng = np.random.default_rng(nb * 3 + M)
    ld = (K + 15) // 16 * 16
    A = np.zeros((nb, M, ld), np.uint16)
    A[:, :, :K] = rng.integers(0, 32769, (nb, M, K))
    A[0, 0, :K] = 32768
    A[0, 1, :K] = 32640
    A[0, 2, :K] = 0
    A[:, :, K:] = 12345  # garbage in the pad must be ignored
    B = np.zeros((nb, N, ld), np.int8)
    B[:, :, :K] = rng.integers(-128, 128, (nb, N, K))
    B[0, 0, :K] = -128
    B[0, 1, :K] = 127
    B[:, :, K:] = 77
    C = torch.empty(nb, M, N, dtype=torch.int32, device="cuda")
    H.call("ivit_bmm_nt_u16i8", P(dev(A.view(np.int16))), P(dev(B)), P(C), nb, M, N, K, ld, ld, N,
           M * ld, N * ld, M * N)
    ref = np.einsum("bmk,bnk->bmn", A[:, :, :K].astype(np.int64), B[:, :, :K].astype(np.int64))
    ref = ((ref + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)  # int32 wrap-around semantics
    assert np.array_equal(C.cpu().numpy(), ref)


@pytest.mark.parametrize("M,N,K", [(300, 256, 128), (257, 136, 64)])
def test_linear_requant_saturating_and_tie_channels(H, M, N, K):
    """requant factors far outside the magic-number range (|z*c| >= 2^31: the kernel must fall back to the
    saturating rint form for those column blocks), int32-scale biases, and factors of exactly 0.5 / 1.5
    (every odd accumulator is a rounding tie) — all against the oracle."""
    from oracle import oracle as orc
    rng = np.random.default_rng(7 * M + N + K)
    x = rng.integers(-128, 128, (M, K), dtype=np.int8)
    w = rng.integers(-128, 128, (N, K), dtype=np.int8)
    b = rng.integers(-2 ** 30, 2 ** 30, N).astype(np.int32)
    b[::3] = rng.integers(-2 ** 10, 2 ** 10, len(b[::3]))
    acc = orc.linear_i8(x, w, b)
    s_out = np.float32(1.0)
    s_pre = np.full(N, 1e-5, np.float32)
    s_pre[0::4] = 0.5            # exact ties
    s_pre[1::4] = 1.5
    s_pre[2::8] = 3.0e4          # |z*c| up to ~2^45: saturates, must not wrap
    s_pre[130:] = 1e-6           # second column block: small factors only where the biases are small
    xd, wd, bd = dev(x), dev(w), dev(b)
    for bits in (8, 16):
        d = iv.freeze.dyadic(s_pre, s_out)
        out = torch.empty(M, N, dtype={8: torch.int8, 16: torch.int16}[bits], device="cuda")
        H.call("ivit_linear_i8_requant", P(xd), P(wd), P(bd), P(dev(d)), bits, P(out), M, N, K)
        ref = orc.requant(acc, orc.dyadic(s_pre, s_out), bits)
        assert np.array_equal(out.cpu().numpy().astype(np.int32), ref), (bits, M, N, K)


@pytest.mark.parametrize("B,Hh,T", [(2, 3, 197), (1, 2, 17), (3, 1, 64), (1, 2, 577), (2, 2, 200), (1, 1, 250)])
def test_fused_attention_equals_unfused_chain(H, B, Hh, T):
    """fused kernel == qk_requant + shiftmax + pv_requant (themselves golden-pinned)."""
    rng = np.random.default_rng(T * 13 + B)
    dh, ld = 64, (T + 15) // 16 * 16
    q = rng.integers(-128, 128, (B * Hh, T, dh), dtype=np.int8)
    k = rng.integers(-128, 128, (B * Hh, T, dh), dtype=np.int8)
    k = (k.astype(np.int32) // 2).astype(np.int8)
    if T > 20:
        k[:, 5] = q[:, 7] // 2 + 60  # peaky rows
    vt = np.zeros((B * Hh, dh, ld), np.int8)
    vt[:, :, :T] = rng.integers(-128, 128, (B * Hh, dh, T))
    s1 = np.float32(0.034)
    zmax = np.abs(np.einsum("bik,bjk->bij", q.astype(np.int32), k.astype(np.int32))).max()
    s_qk = np.float32(np.float32(s1 * s1) * np.float32(0.125))
    s_att = np.float32(zmax * s_qk / 127.0)
    d_qk = iv.freeze.dyadic(s_qk, s_att)
    d_pv = iv.freeze.dyadic(np.float32(np.float32(2.0 ** -15) * s1), np.float32(0.017))
    qd, kd, vd = dev(q), dev(k), dev(vt)
    s8 = torch.zeros(B * Hh, T, ld, dtype=torch.int8, device="cuda")
    p16 = torch.zeros(B * Hh, T, ld, dtype=torch.int16, device="cuda")
    c_ref = torch.zeros(B, T, Hh * dh, dtype=torch.int8, device="cuda")
    c_fus = torch.zeros(B, T, Hh * dh, dtype=torch.int8, device="cuda")
    H.call("ivit_attn_qk_requant", P(qd), P(kd), dyv(d_qk), P(s8), B * Hh, T, dh, ld)
    H.call("ivit_shiftmax", P(s8), B * Hh * T, T, ld, float(s_att), 16, P(p16), ld)
    H.call("ivit_attn_pv_requant", P(p16), P(vd), dyv(d_pv), P(c_ref), B, Hh, T, dh, ld, ld)
    H.call("ivit_attention_fused", P(qd), P(kd), P(vd), dyv(d_qk), float(s_att), dyv(d_pv), P(c_fus), B, Hh, T, dh, ld)
    a, bb = c_ref.cpu().numpy(), c_fus.cpu().numpy()
    assert np.abs(a.astype(np.int32)).max() > 20, "degenerate test data"
    assert np.array_equal(a, bb), f"{(a != bb).sum()} / {a.size} differ"


def _engine_for(g):
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    w = iv.make_vit_weights(cfg, int(g["seed"]))
    from ivit_amd.engine import ViTEngine
    return cfg, w, ViTEngine.from_float(cfg, w, golden_scales(g))


@pytest.mark.parametrize("fname", ["micro_vit_b2.npz", "micro_vit2h_b3.npz", "deit_tiny_b1.npz",
                                   "deit_small_b4.npz", "deit_base_b2.npz", "vit_base_384_b1.npz"])
def test_vit_forward_golden_logits(fname):
    g = load_golden(fname)
    cfg, w, eng = _engine_for(g)
    imgs = iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"]))
    d_imgs = dev(imgs)
    logits = eng.forward(d_imgs).cpu().numpy()                 # native runner, one C call
    assert np.array_equal(logits, g["logits_int"])
    assert np.array_equal(eng.head_scale(), g["logits_scale"])
    # one C-ABI call per operator from Python: same integers
    assert np.array_equal(eng.forward_ops(d_imgs).cpu().numpy(), g["logits_int"])
    if fname == "deit_small_b4.npz":
        # round 6: the D = 384, dh = 64 model takes norm1 inside the qkv GEMM's prologue; the two-launch form gives the same integers
        assert eng._qkv_prepared and eng.fuse_ln_qkv and eng.fuse_ln_mlp and eng.fuse_patch_embed
        eng.fuse_ln_qkv = eng.fuse_ln_mlp = eng.fuse_patch_embed = False       # every layer as its own launches: the same integers
        assert np.array_equal(eng.forward_ops(d_imgs).cpu().numpy(), g["logits_int"])
    else:
        assert not eng._qkv_prepared


@pytest.mark.parametrize("fname,batch,nslices", [("deit_tiny_b1.npz", 5, 2), ("micro_vit2h_b3.npz", 7, 3),
                                                   ("deit_small_b4.npz", 8, 4)])
def test_native_runner_slices_and_graph(fname, batch, nslices):
    """ivit_vit_forward with the batch cut into slices on internal streams, and the hipGraph of it,
    give the integers of the single-stream forward (ragged slice sizes included)."""
    g = load_golden(fname)
    cfg, w, eng = _engine_for(g)
    imgs = np.concatenate([iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"])),
                           iv.make_images_int8(cfg, batch, seed=7)])[:batch]
    d_imgs = dev(imgs)
    ref = eng.forward(d_imgs).cpu().numpy()
    nb = min(batch, int(g["batch"]))
    assert np.array_equal(ref[:nb], g["logits_int"][:nb])
    assert np.array_equal(eng.forward(d_imgs, nslices=nslices).cpu().numpy(), ref)
    replay = eng.capture(d_imgs, nslices)
    for _ in range(3):
        out = replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref)
    # concurrency stress: kernels of different slices overlap on the chip; any LDS / DMA ordering bug in a
    # kernel shows up as a sporadic mismatch here long before it does on one stream
    for it in range(25):
        assert np.array_equal(eng.forward(d_imgs, nslices=nslices).cpu().numpy(), ref), it


def test_native_runner_rejects_bad_workspace():
    import ctypes
    g = load_golden("micro_vit_b2.npz")
    cfg, w, eng = _engine_for(g)
    d_imgs = dev(iv.make_images_int8(cfg, 2, 1))
    lib = eng.h.lib
    n = ctypes.c_size_t()
    assert lib.ivit_vit_workspace_bytes(eng.model, 2, 1, ctypes.byref(n)) == 0 and n.value > 0
    assert lib.ivit_vit_workspace_bytes(eng.model, 2, 3, ctypes.byref(n)) != 0      # more slices than images
    ws = torch.empty(1024, dtype=torch.uint8, device="cuda")
    out = torch.empty(2, cfg.num_classes, dtype=torch.int32, device="cuda")
    st = lib.ivit_vit_forward(eng.model, P(d_imgs), 2, 1, P(ws), 1024, P(out))
    assert st != 0 and b"workspace" in lib.ivit_last_error(eng.h.h)


def test_vit_forward_vs_oracle_residual_stream():
    """final residual stream + logits vs the CPU oracle on a fresh image seed."""
    from oracle import oracle as orc
    g = load_golden("deit_tiny_b1.npz")
    cfg, w, eng = _engine_for(g)
    imgs = iv.make_images_int8(cfg, 3, seed=99)
    o = orc.OracleViT(cfg, w, golden_scales(g))
    cap = {}
    ref_logits, _ = o.forward(imgs, cap)
    logits = eng.forward_ops(dev(imgs)).cpu().numpy()
    x_last = eng.last_x.cpu().numpy().reshape(3, cfg.num_tokens, cfg.embed_dim)
    assert np.array_equal(eng.forward(dev(imgs)).cpu().numpy(), logits)
    assert np.array_equal(x_last, cap[f"blocks.{cfg.depth - 1}.qact4"].astype(np.int16))
    assert np.array_equal(logits, ref_logits)


@pytest.mark.parametrize("fname", ["micro_vit2h_b3.npz", "deit_tiny_b1.npz"])
def test_operator_surface_model_golden(fname):
    """the reference-shaped module chain (one C-ABI call per operator) reproduces the
    reference's integers: every captured site (micro) / final logits (DeiT-T)."""
    g = load_golden(fname)
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    m = iv.VisionTransformer(img_size=cfg.img_size, patch_size=cfg.patch_size, num_classes=cfg.num_classes,
                             embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=4)
    m.load_float_weights(iv.make_vit_weights(cfg, int(g["seed"]))).load_act_scales(golden_scales(g))
    iv.freeze_model(m)
    imgs = iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"]))
    cap = {}
    hooks = []
    if fname.startswith("micro"):
        for name, mod in m.named_modules():
            if f"site/{name}" in g.files:
                hooks.append(mod.register_forward_hook(lambda mod, i, o, name=name: cap.__setitem__(name, o[0])))
    with torch.no_grad():
        acc, scale = m(dev(imgs))
    assert np.array_equal(acc.cpu().numpy(), g["logits_int"])
    assert np.array_equal(scale.numpy(), g["logits_scale"])
    for name, t in cap.items():
        ref = g["site/" + name]
        got = t.cpu().numpy()
        if name == "patch_embed.proj":
            got = got.reshape(got.shape[0], got.shape[1], -1).transpose(0, 2, 1)
        if name == "norm":
            got = got[:, 0]
        assert np.array_equal(got.reshape(ref.shape).astype(np.float64), ref.astype(np.float64)), name
    # the fused engine compiled from the same module agrees too
    eng = m.compile()
    assert np.array_equal(eng.forward(dev(imgs)).cpu().numpy(), g["logits_int"])


def test_operator_error_behaviour():
    """same exceptions as the reference constructors (quant_modules.py:46-48,143-145,77)"""
    with pytest.raises(NotImplementedError):
        iv.QuantLinear(8, 8, quant_mode="asymmetric")
    with pytest.raises(ValueError):
        iv.QuantLinear(8, 8, quant_mode="none")
    with pytest.raises(NotImplementedError):
        iv.QuantAct(quant_mode="asymmetric")
    with pytest.raises(ValueError):
        iv.QuantAct(quant_mode="bogus")
    lin = iv.QuantLinear(64, 16, per_channel=False)
    with pytest.raises(Exception):
        lin(torch.zeros(4, 64, dtype=torch.int8, device="cuda"), torch.tensor(0.1))
    act = iv.QuantAct()
    act.fix()             # frozen without ever having seen a range or a loaded scale
    with pytest.raises(ValueError):
        act(torch.zeros(4, 8, dtype=torch.int32, device="cuda"), torch.tensor(0.1))


@pytest.mark.parametrize("fname", ["micro_swin_b2.npz", "swin_tiny_b1.npz"])
def test_swin_operator_surface_golden(fname):
    """Swin on the operator surface (windowed attention dh=32, 8-bit masked Shiftmax, rel-pos bias,
    patch merging, avg-pool) reproduces the reference: every site (micro) / logits (Swin-T)."""
    from ivit_amd.swin_quant import SwinTransformer
    g = load_golden(fname)
    cfg = iv.SWIN_CONFIGS[str(g["cfg_name"])]
    m = SwinTransformer(img_size=cfg.img_size, patch_size=cfg.patch_size, num_classes=cfg.num_classes,
                        embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads,
                        window_size=cfg.window_size, mlp_ratio=cfg.mlp_ratio)
    m.load_float_weights(iv.make_swin_weights(cfg, int(g["seed"]))).load_act_scales(golden_scales(g))
    iv.freeze_model(m)
    imgs = iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"]))
    cap = {}
    if fname.startswith("micro"):
        for name, mod in m.named_modules():
            if f"site/{name}" in g.files:
                mod.register_forward_hook(lambda mod, i, o, name=name: cap.__setitem__(name, o[0]))
    with torch.no_grad():
        acc, scale = m(dev(imgs))
    for name, t in cap.items():
        ref = g["site/" + name]
        got = t.cpu().numpy()
        if name == "patch_embed.proj":
            got = got.reshape(got.shape[0], got.shape[1], -1).transpose(0, 2, 1)
        assert np.array_equal(got.reshape(ref.shape).astype(np.float64), ref.astype(np.float64)), name
    assert np.array_equal(acc.cpu().numpy(), g["logits_int"])
    assert np.array_equal(scale.numpy(), g["logits_scale"])


# ---------------------------------------------------------------- Swin engine (fused windowed attention)
@pytest.mark.parametrize("fname", ["micro_swin_b2.npz", "swin_tiny_b1.npz"])
def test_swin_engine_golden_logits(fname):
    """SwinEngine (natural-order activations, ivit_window_attention_fused) reproduces the reference's
    int32 logits; on the micro model also against the CPU oracle for a fresh batch."""
    from ivit_amd.swin_engine import SwinEngine
    g = load_golden(fname)
    cfg = iv.SWIN_CONFIGS[str(g["cfg_name"])]
    w = iv.make_swin_weights(cfg, int(g["seed"]))
    eng = SwinEngine(cfg, w, golden_scales(g))
    imgs = iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"]))
    logits = eng.forward(dev(imgs)).cpu().numpy()                    # native runner (ivit_swin_forward)
    assert np.array_equal(logits, g["logits_int"])
    assert np.array_equal(eng.head_scale, g["logits_scale"])
    assert np.array_equal(eng.forward_ops(dev(imgs)).cpu().numpy(), g["logits_int"])   # one C-ABI call per operator
    if fname.startswith("micro"):
        from oracle import oracle as orc
        imgs2 = iv.make_images_int8(cfg, 5, seed=123)
        ref, _ = orc.OracleSwin(cfg, w, golden_scales(g)).forward(imgs2)
        assert np.array_equal(eng.forward(dev(imgs2)).cpu().numpy(), ref)
    # the table form of the windowed attention (off by default: not faster on MI355X) through both runners
    eng_t = SwinEngine(cfg, w, golden_scales(g), exp_tables=True)
    assert any(k.endswith("attn.exp_aq") for k in eng_t.table)
    assert np.array_equal(eng_t.forward(dev(imgs)).cpu().numpy(), g["logits_int"])
    assert np.array_equal(eng_t.forward_ops(dev(imgs)).cpu().numpy(), g["logits_int"])


@pytest.fixture(scope="module")
def mlp_production_case():
    """Operands of one fused Mlp (384 -> 1536 -> 384) over 50432 tokens and the ORACLE's output for them
    (oracle/ivit_twin.c chains the restated operators: layers_quant.py:144-153 + vit_quant.py:141-142).  The operator is
    row-wise, so the oracle's first M rows are the oracle's answer for the first M rows alone: one 50432-row CPU run (~20 s on
    the GPU box's host) serves every row count below."""
    from abi_cases import load_twin
    twin = load_twin()
    hp = lambda a: a.ctypes.data_as(_P)
    dyv = lambda d: _lib.Dyadic(float(d[0, 0]), float(d[0, 1]))
    M = 50432
    rng = np.random.default_rng(M)
    C, Hd = 384, 1536
    c = dict(M=M, C=C, Hd=Hd, dyv=dyv)
    c["x"] = rng.integers(-128, 128, (M, C), dtype=np.int8)
    c["w1"] = np.rint(rng.normal(0, 40, (Hd, C)).clip(-127, 127)).astype(np.int8); c["b1"] = rng.integers(-2000, 2000, Hd).astype(np.int32)
    c["w2"] = np.rint(rng.normal(0, 40, (C, Hd)).clip(-127, 127)).astype(np.int8); c["b2"] = rng.integers(-2000, 2000, C).astype(np.int32)
    c["d1"] = iv.freeze.dyadic((10 ** rng.uniform(-5.6, -5.3, Hd)).astype(np.float32), np.float32(0.04))
    c["d2"] = iv.freeze.dyadic((10 ** rng.uniform(-5.9, -5.6, C)).astype(np.float32), np.float32(2e-4))
    c["dm"], c["dr"] = iv.freeze.dyadic(np.float32(2e-4), np.float32(2.5e-4)), iv.freeze.dyadic(np.float32(3e-4), np.float32(2.5e-4))
    c["res"] = rng.integers(-20000, 20000, (M, C)).astype(np.int16)
    c["dg"] = iv.freeze.dyadic(np.float32(0.04 * 2.0 ** -7), np.float32(0.03))
    tab = np.zeros(65536, np.int8)
    assert twin.ivit_cpu_shiftgelu_build_table(None, 0.04, dyv(c["dg"]), hp(tab)) == 0
    c1, c2, cm = (_P() for _ in range(3))
    assert twin.ivit_cpu_linear_plan_create(None, hp(c["w1"]), hp(c["b1"]), hp(c["d1"]), Hd, C, ctypes.byref(c1)) == 0
    assert twin.ivit_cpu_linear_plan_create(None, hp(c["w2"]), hp(c["b2"]), hp(c["d2"]), C, Hd, ctypes.byref(c2)) == 0
    assert twin.ivit_cpu_mlp_plan_create(None, c1, c2, ctypes.byref(cm)) == 0
    oc = np.zeros((M, C), np.int16)
    assert twin.ivit_cpu_mlp_fused_planned(None, cm, hp(c["x"]), hp(tab), dyv(c["dm"]), dyv(c["dr"]), hp(c["res"]), hp(oc), M) == 0
    twin.ivit_cpu_mlp_plan_destroy(cm)
    for pl in (c1, c2):
        twin.ivit_cpu_linear_plan_destroy(pl)
    c["oracle"] = oc
    return c


@pytest.mark.parametrize("M", [80 * 256 - 1, 80 * 256 + 1, 25216, 40961, 50176, 50432])
def test_mlp_fused_planned_vs_oracle_production_geometry(M, mlp_production_case):
    """the dominant kernel against the ORACLE, not against the HIP chain, at the row counts the headline run
    produces: 25216 (a half-batch slice of DeiT-S b256) and 80 * 256 -+ 1 (one 5-tile unit per workgroup, one row short /
    one row over: 4- and 5-tile units, clamped rows, the balanced and the round-robin schedule).
    Round 6: the THREE-units-per-CU geometry of the role-split kernel — 50432 (the whole
    DeiT-S b256 batch: units of 5 / 4 / 4 tiles, a MIDDLE unit whose producers run beside the consumers of the unit before while
    the slice counters of the unit before that are already consumed), 50176 (units of 4 / 4 / 5: the NT = 2 -> 3 switch inside
    one workgroup) and 40961 (two 5-tile units everywhere, exactly one workgroup with a third, one-row unit).  The output buffer
    has a guard row behind row M - 1 that must stay untouched."""
    c = mlp_production_case
    C, Hd, dyv = c["C"], c["Hd"], c["dyv"]
    H = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    tabd = torch.empty(65536, dtype=torch.int8, device="cuda")
    H.call("ivit_shiftgelu_build_table", 0.04, dyv(c["dg"]), _P(tabd.data_ptr()))
    d = {k: torch.from_numpy(np.ascontiguousarray(c[k][:M] if k in ("x", "res") else c[k])).cuda() for k in ("x", "w1", "b1", "w2", "b2", "d1", "d2", "res")}
    g1, g2, gm = (_P() for _ in range(3))
    H.call("ivit_linear_plan_create", _P(d["w1"].data_ptr()), _P(d["b1"].data_ptr()), _P(d["d1"].data_ptr()), Hd, C, ctypes.byref(g1))
    H.call("ivit_linear_plan_create", _P(d["w2"].data_ptr()), _P(d["b2"].data_ptr()), _P(d["d2"].data_ptr()), C, Hd, ctypes.byref(g2))
    H.call("ivit_mlp_plan_create", g1, g2, ctypes.byref(gm))
    oc = c["oracle"][:M]
    # round 5: the plan owns two kernels (lock-step ivit_mlp.h, role-split ivit_mlp_rs.h); 0 = the shape-based default
    for kernel in (0, 1, 2):
        assert H.lib.ivit_mlp_plan_select(gm, kernel) == 0
        og = torch.full((M + 1, C), 0x5555, dtype=torch.int16, device="cuda")
        H.call("ivit_mlp_fused_planned", gm, _P(d["x"].data_ptr()), _P(tabd.data_ptr()), dyv(c["dm"]), dyv(c["dr"]), _P(d["res"].data_ptr()), _P(og.data_ptr()), M)
        got = og.cpu().numpy()
        assert np.array_equal(got[:M], oc), (kernel, int((got[:M] != oc).sum()))
        assert (got[M] == 0x5555).all(), (kernel, "wrote behind the last row")
    assert H.lib.ivit_mlp_plan_select(gm, 3) == 1 and H.lib.ivit_mlp_plan_select(None, 0) == 1
    H.lib.ivit_mlp_plan_destroy(gm)
    for pl in (g1, g2):
        H.lib.ivit_linear_plan_destroy(pl)


@pytest.mark.parametrize("M", [80 * 256 + 1, 25216, 40961, 50176, 50432, 100000])
def test_layernorm_mlp_fused_equals_two_launches(M, mlp_production_case):
    """norm2 + qact3 in the head of the fused Mlp's launch (ivit_layernorm_mlp_fused_planned, mlp384rs_kernel<.., LNH>; vit_quant.py:139-142)
    == ivit_layernorm_requant followed by ivit_mlp_fused_planned (both pinned against the oracle above), bit for bit, on the 16-bit stream
    that is LayerNorm input AND identity branch: the balanced and the round-robin unit schedules, ragged last rows, guard rows behind the
    output and behind the scratch; refused (nothing launched) where the launch would run on the lock-step kernel."""
    c = mlp_production_case
    C, Hd, dyv = c["C"], c["Hd"], c["dyv"]
    H = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(M)
    tabd = torch.empty(65536, dtype=torch.int8, device="cuda")
    H.call("ivit_shiftgelu_build_table", 0.04, dyv(c["dg"]), _P(tabd.data_ptr()))
    d = {k: torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("w1", "b1", "w2", "b2", "d1", "d2")}
    x16 = rng.integers(-20000, 20000, (M, C)).astype(np.int16)
    x16[:, : C // 2] //= 64
    x16 = torch.from_numpy(x16).cuda()
    wln = rng.normal(1.0, 0.4, C).astype(np.float32) * rng.choice([-1.0, 1.0], C).astype(np.float32)
    bias_int, sc = iv.freeze.layernorm_constants(wln, rng.normal(0.0, 0.5, C).astype(np.float32))
    s_in = np.float32(2.5e-4)
    bi_d, sc_d = torch.from_numpy(bias_int).cuda(), torch.from_numpy(sc).cuda()
    dln = torch.from_numpy(iv.freeze.dyadic(sc, np.float32(0.031))).cuda()
    g1, g2, gm = (_P() for _ in range(3))
    H.call("ivit_linear_plan_create", _P(d["w1"].data_ptr()), _P(d["b1"].data_ptr()), _P(d["d1"].data_ptr()), Hd, C, ctypes.byref(g1))
    H.call("ivit_linear_plan_create", _P(d["w2"].data_ptr()), _P(d["b2"].data_ptr()), _P(d["d2"].data_ptr()), C, Hd, ctypes.byref(g2))
    H.call("ivit_mlp_plan_create", g1, g2, ctypes.byref(gm))
    a8 = torch.empty(M, C, dtype=torch.int8, device="cuda")
    H.call("ivit_layernorm_requant", _P(x16.data_ptr()), M, C, C, float(s_in), _P(bi_d.data_ptr()), _P(sc_d.data_ptr()), _P(dln.data_ptr()), _P(a8.data_ptr()))
    want = torch.full((M + 1, C), 0x5555, dtype=torch.int16, device="cuda")
    H.call("ivit_mlp_fused_planned", gm, _P(a8.data_ptr()), _P(tabd.data_ptr()), dyv(c["dm"]), dyv(c["dr"]), _P(x16.data_ptr()), _P(want.data_ptr()), M)
    got = torch.full((M + 1, C), 0x5555, dtype=torch.int16, device="cuda")
    scratch = torch.full((M + 1, C), 77, dtype=torch.int8, device="cuda")
    args = (gm, _P(x16.data_ptr()), float(s_in), _P(bi_d.data_ptr()), _P(sc_d.data_ptr()), _P(dln.data_ptr()), _P(scratch.data_ptr()), _P(tabd.data_ptr()),
            dyv(c["dm"]), dyv(c["dr"]), _P(got.data_ptr()), M)
    H.call("ivit_layernorm_mlp_fused_planned", *args)
    assert torch.equal(got, want), int((got != want).sum())
    assert torch.equal(scratch[:M], a8) and (scratch[M] == 77).all() and len(torch.unique(want)) > 5000
    # the same launch sized for a share of the CUs (ivit_set_cu_share: what the runners give the handle of a slice): same integers
    for cus in (128, 100, 7):
        H.set_cu_share(cus)
        got.fill_(0x5555)
        try:
            H.call("ivit_layernorm_mlp_fused_planned", *args)
        finally:
            H.set_cu_share(0)
        assert torch.equal(got, want), (cus, int((got != want).sum()))
    assert H.lib.ivit_mlp_plan_select(gm, 1) == 0            # pinned to the lock-step kernel: refused
    with pytest.raises(_lib.IvitError, match="role-split"):
        H.call("ivit_layernorm_mlp_fused_planned", *args)
    H.lib.ivit_mlp_plan_destroy(gm)
    for pl in (g1, g2):
        H.lib.ivit_linear_plan_destroy(pl)


# ---------------------------------------------------------------- calibration
CALIB_BATCH = {"micro_vit_b2.npz": 4, "micro_vit2h_b3.npz": 4, "deit_tiny_b1.npz": 2, "micro_swin_b2.npz": 4}
# What is pinned per fixture (measured with tools/calib_diag.py): the FIRST QuantAct site, in forward order, whose calibrated
# scale differs from the reference's, how many sites before it are bit-equal, a bound on the largest relative scale
# difference anywhere, and a bound on |float logit here - float logit reference| on the fixture's images.
# Round 4: the ShiftGELU-fed sites (`mlp.qact1`) track the reference's own fp32 value fl(fl(x_int * sigmoid_int) * s) with
# the non-integer x_int = fl(fl(Q s) / s) (IntGELU.calibrating) — elementwise, deterministic, reproduced exactly: DeiT-T
# (136 sites) and micro-Swin (59) are now bit-equal everywhere, logits included.  What remains is the one site class that
# is not deterministic in the reference itself: `attn.qact2` behind the fp32 bmm attn.v of non-integers (vit_quant.py:79),
# whose last bits follow the host BLAS's summation order.
CALIB_PIN = {
    "micro_vit_b2.npz": (None, 26, 0.0, 0.0),
    "micro_vit2h_b3.npz": ("blocks.1.attn.qact2", 17, 3e-7, 0.0),
    "deit_tiny_b1.npz": (None, 136, 0.0, 0.0),
    "micro_swin_b2.npz": (None, 59, 0.0, 0.0),
}


@pytest.mark.parametrize("fname", sorted(CALIB_BATCH))
def test_calibration_reproduces_reference_scales(fname):
    """running_stat=True branch of QuantAct (quant_modules.py:170-192): one forward of the seeded fp32 calibration batch
    through the operator surface, then freeze_model.  Pinned against the reference's own calibration (the scales stored in
    the fixtures): bit-equal scales at every site up to the named first site of CALIB_PIN (None: every site, and then the
    int32 logits of the fixture's images too), the bound on the scale differences after it, equal arg-max and the bound
    on the float logits."""
    g = load_golden(fname)
    name = str(g["cfg_name"])
    if name in iv.SWIN_CONFIGS:
        from ivit_amd.swin_quant import SwinTransformer
        cfg = iv.SWIN_CONFIGS[name]
        m = SwinTransformer(img_size=cfg.img_size, patch_size=cfg.patch_size, in_chans=cfg.in_chans,
                            num_classes=cfg.num_classes, embed_dim=cfg.embed_dim, depths=cfg.depths,
                            num_heads=cfg.num_heads, window_size=cfg.window_size, mlp_ratio=cfg.mlp_ratio)
        m.load_float_weights(iv.make_swin_weights(cfg, int(g["seed"])))
    else:
        cfg = iv.CONFIGS[name]
        m = iv.VisionTransformer(img_size=cfg.img_size, patch_size=cfg.patch_size, num_classes=cfg.num_classes,
                                 embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=4)
        m.load_float_weights(iv.make_vit_weights(cfg, int(g["seed"])))
    order = []
    for n, mod in m.named_modules():
        if type(mod) is iv.QuantAct:
            mod.register_forward_hook(lambda mod, i, o, n=n: order.append(n) if n not in order else None)
    calib = iv.make_calibration_batch(cfg, CALIB_BATCH[fname])
    with torch.no_grad():
        m(dev(calib))
    iv.freeze_model(m)
    ref = golden_scales(g)
    got = {k: np.float32(mod.act_scaling_factor.reshape(-1)[0].item()) for k, mod in m.named_modules()
           if type(mod) is iv.QuantAct}
    assert all(k in got for k in ref), set(ref) - set(got)
    sites = [k for k in order if k in ref and ref[k] > 0]
    diff = [k for k in sites if got[k] != ref[k]]
    first, n_equal, rel_bound, logit_bound = CALIB_PIN[fname]
    assert (diff[0] if diff else None) == first, (diff[:3], first)
    assert (sites.index(first) if first else len(sites)) == n_equal
    assert max(abs(float(got[k]) - float(ref[k])) / float(ref[k]) for k in sites) <= rel_bound
    imgs = iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"]))
    with torch.no_grad():
        acc, sc = m(dev(imgs))
    here = acc.cpu().numpy().astype(np.float64) * np.asarray(sc, np.float64)
    there = g["logits_int"].astype(np.float64) * g["logits_scale"].astype(np.float64)
    assert np.array_equal(here.argmax(1), there.argmax(1))
    assert np.abs(here - there).max() <= logit_bound
    if not diff:
        assert np.array_equal(acc.cpu().numpy(), g["logits_int"])


def test_calibration_through_the_fake_quant_surface():
    """the same calibration with the model on the reference's fp32 fake-quant tensors (VisionTransformer.fake_quant):
    the QuantAct behind ShiftGELU must track the reference's own fp32 value there too (IntGELU's `_calib_fp32` rides on the
    fake-quant tensor), so every scale of the micro-ViT fixture is bit-equal to the reference's on this path as well."""
    g = load_golden("micro_vit_b2.npz")
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    m = iv.VisionTransformer(img_size=cfg.img_size, patch_size=cfg.patch_size, num_classes=cfg.num_classes,
                             embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=4)
    m.load_float_weights(iv.make_vit_weights(cfg, int(g["seed"])))
    m.fake_quant = True
    with torch.no_grad():
        m(dev(iv.make_calibration_batch(cfg, CALIB_BATCH["micro_vit_b2.npz"])))
    iv.freeze_model(m)
    ref = golden_scales(g)
    got = {k: np.float32(mod.act_scaling_factor.reshape(-1)[0].item()) for k, mod in m.named_modules() if type(mod) is iv.QuantAct}
    diff = [k for k in ref if ref[k] > 0 and k in got and got[k] != ref[k]]
    assert not diff, diff[:4]


def test_imported_reference_state_dict_runs_to_golden_logits():
    """checkpoint importer: the reference's post-forward state dict -> this build's
    operator chain and fused engine -> the reference's logits."""
    from ivit_amd import checkpoint as ck
    f = load_golden("micro_vit_state_dict.npz")
    g = load_golden("micro_vit_b2.npz")
    cfg = iv.CONFIGS[str(f["cfg_name"])]
    w = iv.make_vit_weights(cfg, int(f["seed"]))
    sd = {str(k): torch.from_numpy(np.asarray(w[str(k)] if str(k) in w else f["buf/" + str(k)]).copy()) for k in f["keys"]}
    m = iv.VisionTransformer(img_size=cfg.img_size, patch_size=cfg.patch_size, num_classes=cfg.num_classes,
                             embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=4)
    ck.load_reference_state_dict(m, {"state_dict": sd})
    imgs = iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"]))
    with torch.no_grad():
        acc, _ = m(dev(imgs))
    assert np.array_equal(acc.cpu().numpy(), g["logits_int"])
    assert np.array_equal(m.compile().forward(dev(imgs)).cpu().numpy(), g["logits_int"])


def test_full_size_batch_properties_deit_small_b256():
    """BASELINE config 2 at full size (DeiT-S, 256 images): the oracle is too slow here, so parity rides on
    size-independent properties — images are independent, so (i) the golden 4-image prefix is reproduced
    inside the big batch, (ii) permuting the batch permutes the logits, (iii) duplicated images give
    duplicated logits, (iv) slices / hipGraph give the same integers as one stream."""
    g = load_golden("deit_small_b4.npz")
    cfg, w, eng = _engine_for(g)
    B = 256
    imgs = np.concatenate([iv.make_images_int8(cfg, 4, int(g["images_seed"])), iv.make_images_int8(cfg, B - 4, seed=11)])
    imgs[200:204] = imgs[0:4]                                  # duplicates
    d = dev(imgs)
    ref = eng.forward(d).cpu().numpy()
    assert np.array_equal(ref[:4], g["logits_int"])
    assert np.array_equal(ref[200:204], ref[0:4])
    perm = np.random.default_rng(5).permutation(B)
    out_p = eng.forward(dev(imgs[perm])).cpu().numpy()
    assert np.array_equal(out_p, ref[perm])
    assert np.array_equal(eng.forward(d, nslices=4).cpu().numpy(), ref)
    rep = eng.capture(d, 4)
    out = rep()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref)
    _oracle_sample_check(cfg, w, golden_scales(g), imgs, ref, 32, first_free=4)


def _oracle_sample_check(cfg, w, scales, imgs, ref, count, first_free, swin=False):
    """a random sample of NON-golden images of a full-size batch against the CPU oracle
    (oracle/ivit_oracle.c through OracleViT / OracleSwin, ~6 DeiT-S images per second on the GPU box's host) — the
    properties above only ever compare those images with the HIP path itself."""
    from oracle import oracle as orc
    idx = np.sort(np.random.default_rng(2026).choice(np.arange(first_free, len(imgs)), size=count, replace=False))
    o = (orc.OracleSwin if swin else orc.OracleViT)(cfg, w, scales)
    want, _ = o.forward(np.ascontiguousarray(imgs[idx]))
    assert np.array_equal(ref[idx], np.asarray(want)), "HIP logits of sampled batch images differ from the oracle"


def test_full_size_batch_properties_swin_tiny_b64():
    """Swin-T at a large batch: golden image inside the batch, permutation equivariance."""
    from ivit_amd.swin_engine import SwinEngine
    g = load_golden("swin_tiny_b1.npz")
    cfg = iv.SWIN_CONFIGS[str(g["cfg_name"])]
    eng = SwinEngine(cfg, iv.make_swin_weights(cfg, int(g["seed"])), golden_scales(g))
    B = 64
    imgs = np.concatenate([iv.make_images_int8(cfg, 1, int(g["images_seed"])), iv.make_images_int8(cfg, B - 1, seed=12)])
    ref = eng.forward(dev(imgs)).cpu().numpy().copy()
    assert np.array_equal(ref[:1], g["logits_int"])
    perm = np.random.default_rng(6).permutation(B)
    assert np.array_equal(eng.forward(dev(imgs[perm])).cpu().numpy(), ref[perm])
    # batch slices on separate streams, and the hipGraph of that
    d = dev(imgs)
    assert np.array_equal(eng.forward(d, nslices=3).cpu().numpy(), ref)
    rep = eng.capture(d, 4)
    for _ in range(3):
        out = rep()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref)


def test_act_out_int8_logits_extension():
    """N4: the reference's never-called `act_out` QuantAct as a defined int8-logits epilogue: calibrates from
    the logits, then equals the oracle's per-class dyadic requant of the head accumulators."""
    from oracle import oracle as orc
    g = load_golden("micro_vit2h_b3.npz")
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    m = iv.VisionTransformer(img_size=cfg.img_size, patch_size=cfg.patch_size, num_classes=cfg.num_classes,
                             embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=4)
    m.load_float_weights(iv.make_vit_weights(cfg, int(g["seed"]))).load_act_scales(golden_scales(g))
    iv.freeze_model(m)
    imgs = iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"]))
    with torch.no_grad():
        acc, scale = m(dev(imgs))
        m.act_out.unfix()                       # calibrate this one site from the logits it sees
        q8, s8 = m.int8_logits(acc, scale)
        m.act_out.fix()
        q8b, s8b = m.int8_logits(acc, scale)
    assert np.array_equal(acc.cpu().numpy(), g["logits_int"])
    X = acc.cpu().numpy().astype(np.float32) * g["logits_scale"].astype(np.float32)
    s_ref = iv.freeze.symmetric_scale(X.min(), X.max(), 8)
    assert np.float32(s8.reshape(-1)[0].item()) == np.float32(s_ref)
    ref = orc.requant(g["logits_int"].astype(np.int32), orc.dyadic(g["logits_scale"], np.float32(s_ref)), 8)
    assert np.array_equal(q8.cpu().numpy().astype(np.int32), ref)
    assert np.array_equal(q8b.cpu().numpy(), q8.cpu().numpy()) and q8.dtype == torch.int8
    assert np.abs(q8.cpu().numpy().astype(np.int32)).max() == 127       # the calibrated range is used in full


@pytest.mark.parametrize("M", [64, 1000, 64 * 300 + 17])
def test_mlp_fused_equals_unfused_chain(H, M):
    """ivit_mlp_fused (weights resident in LDS, hidden never in HBM) == fc1+requant -> GELU table -> fc2+requant
    +identity issued as three kernels; ragged last tile included."""
    rng = np.random.default_rng(M)
    C, HD = 96, 384
    x = dev(rng.integers(-128, 128, (M, C), dtype=np.int8))
    w1 = dev(rng.integers(-128, 128, (HD, C), dtype=np.int8)); b1 = dev(rng.integers(-3000, 3000, HD).astype(np.int32))
    w2 = dev(rng.integers(-128, 128, (C, HD), dtype=np.int8)); b2 = dev(rng.integers(-3000, 3000, C).astype(np.int32))
    d1 = dev(iv.freeze.dyadic((10 ** rng.uniform(-5.3, -4.9, HD)).astype(np.float32), np.float32(0.012)))
    d2 = dev(iv.freeze.dyadic((10 ** rng.uniform(-5.6, -5.2, C)).astype(np.float32), np.float32(2e-4)))
    dm = iv.freeze.dyadic(np.float32(2e-4), np.float32(3.1e-4)); dr = iv.freeze.dyadic(np.float32(2.7e-4), np.float32(3.1e-4))
    res = dev(rng.integers(-30000, 30000, (M, C)).astype(np.int16))
    tab = torch.empty(65536, dtype=torch.int8, device="cuda")
    H.call("ivit_shiftgelu_build_table", 0.03, dyv(iv.freeze.dyadic(np.float32(0.03 * 2.0 ** -7), np.float32(0.02))), P(tab))
    h8 = torch.empty(M, HD, dtype=torch.int8, device="cuda"); g8 = torch.empty_like(h8)
    ref = torch.empty(M, C, dtype=torch.int16, device="cuda"); out = torch.full((M, C), -7, dtype=torch.int16, device="cuda")
    H.call("ivit_linear_i8_requant", P(x), P(w1), P(b1), P(d1), 8, P(h8), M, HD, C)
    H.call("ivit_shiftgelu_requant_lut", P(h8), M, HD, P(tab), P(g8))
    H.call("ivit_linear_i8_requant_residual", P(g8), P(w2), P(b2), P(d2), dyv(dm), dyv(dr), P(res), P(ref), M, C, HD)
    H.call("ivit_mlp_fused", P(x), P(w1), P(b1), P(d1), P(tab), P(w2), P(b2), P(d2), dyv(dm), dyv(dr), P(res), P(out), M, C, HD)
    assert np.abs(h8.cpu().numpy().astype(np.int32)).max() >= 127          # the hidden tensor saturates in places
    assert np.array_equal(out.cpu().numpy(), ref.cpu().numpy())
    # unsupported shapes say so instead of running something else
    st = H.lib.ivit_mlp_fused(H.h, P(x), P(w1), P(b1), P(d1), P(tab), P(w2), P(b2), P(d2), dyv(dm), dyv(dr), P(res), P(out), M, 192, 768)
    assert st == 3


@pytest.mark.parametrize("M", [64, 1000, 64 * 300 + 17, 25216, 16 * 256 * 3 + 5])
def test_mlp_fused_planned_equals_unfused_chain(H, M):
    """ivit_mlp_fused_planned (D = 384, hidden = 1536: weights streamed in fragment order, hidden tile in LDS) == the planned
    fc1+requant -> GELU table -> fc2+requant+identity kernels it replaces; ragged last tile, units of 1..5 token tiles
    (25216 tokens = 6.2 tiles per workgroup: units of 3 and 4 tiles); repeated launches."""
    rng = np.random.default_rng(M + 5)
    C, HD = 384, 1536
    x = dev(rng.integers(-128, 128, (M, C), dtype=np.int8))
    w1 = dev(rng.integers(-128, 128, (HD, C), dtype=np.int8)); b1 = dev(rng.integers(-3000, 3000, HD).astype(np.int32))
    w2 = dev(rng.integers(-128, 128, (C, HD), dtype=np.int8)); b2 = dev(rng.integers(-3000, 3000, C).astype(np.int32))
    d1 = dev(iv.freeze.dyadic((10 ** rng.uniform(-5.6, -5.2, HD)).astype(np.float32), np.float32(0.012)))
    d2 = dev(iv.freeze.dyadic((10 ** rng.uniform(-5.9, -5.5, C)).astype(np.float32), np.float32(2e-4)))
    dm = iv.freeze.dyadic(np.float32(2e-4), np.float32(3.1e-4)); dr = iv.freeze.dyadic(np.float32(2.7e-4), np.float32(3.1e-4))
    res = dev(rng.integers(-30000, 30000, (M, C)).astype(np.int16))
    tab = torch.empty(65536, dtype=torch.int8, device="cuda")
    H.call("ivit_shiftgelu_build_table", 0.03, dyv(iv.freeze.dyadic(np.float32(0.03 * 2.0 ** -7), np.float32(0.02))), P(tab))
    p1, p2, mp = _P(), _P(), _P()
    H.call("ivit_linear_plan_create", P(w1), P(b1), P(d1), HD, C, ctypes.byref(p1))
    H.call("ivit_linear_plan_create", P(w2), P(b2), P(d2), C, HD, ctypes.byref(p2))
    H.call("ivit_mlp_plan_create", p1, p2, ctypes.byref(mp))
    try:
        h8 = torch.empty(M, HD, dtype=torch.int8, device="cuda"); g8 = torch.empty_like(h8)
        ref = torch.empty(M, C, dtype=torch.int16, device="cuda")
        H.call("ivit_linear_i8_requant_planned", p1, P(x), 8, P(h8), M)
        H.call("ivit_shiftgelu_requant_lut", P(h8), M, HD, P(tab), P(g8))
        H.call("ivit_linear_i8_requant_residual_planned", p2, P(g8), dyv(dm), dyv(dr), P(res), P(ref), M)
        hh = h8.cpu().numpy().astype(np.int32)
        assert hh.max() == 127 and hh.min() == -128          # the hidden tensor saturates on both sides
        for rep in range(6):                                  # both kernels of the plan (ivit_mlp_plan_select), repeated launches
            assert H.lib.ivit_mlp_plan_select(mp, 1 + rep % 2) == 0
            out = torch.full((M, C), -7, dtype=torch.int16, device="cuda")
            H.call("ivit_mlp_fused_planned", mp, P(x), P(tab), dyv(dm), dyv(dr), P(res), P(out), M)
            assert np.array_equal(out.cpu().numpy(), ref.cpu().numpy()), rep
        assert H.lib.ivit_mlp_plan_select(mp, 0) == 0
        # multipliers outside the fast residual range are refused, not mis-computed
        big = _lib.Dyadic(1024.0, 1.0)
        assert H.lib.ivit_mlp_fused_planned(H.h, mp, P(x), P(tab), big, dyv(dr), P(res), P(out), M) == 3
        # other shapes are refused at plan time
        bad = _P()
        assert H.lib.ivit_mlp_plan_create(H.h, p2, p1, ctypes.byref(bad)) == 3
    finally:
        H.lib.ivit_mlp_plan_destroy(mp)
        H.lib.ivit_linear_plan_destroy(p1)
        H.lib.ivit_linear_plan_destroy(p2)


def test_normalize_quantize_u8_matches_torch_transform_chain():
    """N3 (device part): uint8 HWC -> ToTensor -> Normalize -> input QuantAct == the same chain in torch CPU
    fp32 (what torchvision's ToTensor / Normalize compute), for every pixel value and odd image sizes."""
    from ivit_amd.preprocess import normalize_quantize, IMAGENET_DEFAULT_MEAN as MEAN, IMAGENET_DEFAULT_STD as STD
    rng = np.random.default_rng(3)
    for (B, Hh, W), scale in (((2, 16, 16), 0.0207), ((3, 37, 53), 0.0181), ((1, 224, 224), 0.02078)):
        u = rng.integers(0, 256, (B, Hh, W, 3), dtype=np.uint8)
        u.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
        t = torch.from_numpy(u).permute(0, 3, 1, 2).float().div(255)                       # ToTensor
        mean = torch.tensor(MEAN, dtype=torch.float32).view(1, 3, 1, 1)
        std = torch.tensor(STD, dtype=torch.float32).view(1, 3, 1, 1)
        x = t.sub(mean).div(std)                                                           # Normalize
        inv = np.float32(1.0) / np.float32(scale)
        ref = torch.clamp(torch.round(x * float(inv)), -128, 127).to(torch.int8).numpy()    # quant_utils.py:12-48
        got = normalize_quantize(dev(u), scale).cpu().numpy()
        assert np.array_equal(got, ref), (B, Hh, W)


@pytest.mark.parametrize("spec", [("r0", 48, 16, 64, 1, 1, 10, 3), ("r1", 32, 8, 128, 2, 2, 7, 5), ("r2", 64, 16, 192, 1, 3, 33, 2),
                                  ("r3", 32, 16, 64, 2, 2, 5, 9)])
def test_random_shapes_self_calibrated_engine_vs_oracle(spec):
    """shapes no fixture covers (token counts 5..17, 1..3 heads, head dim 32 -> unfused attention path, odd class
    counts, ragged batches): calibrate on the device, then the native runner (1 and 3 slices) must equal the CPU
    oracle run on the same weights and the calibrated scales."""
    from oracle import oracle as orc
    name, img, patch, D, depth, heads, ncls, B = spec
    cfg = iv.ViTConfig(name, img_size=img, patch_size=patch, num_classes=ncls, embed_dim=D, depth=depth, num_heads=heads)
    w = iv.make_vit_weights(cfg, seed=len(name) + D)
    m = iv.VisionTransformer(img_size=img, patch_size=patch, num_classes=ncls, embed_dim=D, depth=depth, num_heads=heads,
                             mlp_ratio=4)
    m.load_float_weights(w)
    with torch.no_grad():
        m(dev(iv.make_calibration_batch(cfg, 3, seed=17)))
    iv.freeze_model(m)
    scales = {k: v for k, v in m.act_scales().items() if v > 0}
    imgs = iv.make_images_int8(cfg, B, seed=4)
    ref, _ = orc.OracleViT(cfg, w, scales).forward(imgs)
    eng = m.compile()
    assert np.array_equal(eng.forward(dev(imgs)).cpu().numpy(), ref)
    if B >= 3:
        assert np.array_equal(eng.forward(dev(imgs), nslices=3).cpu().numpy(), ref)
    with torch.no_grad():
        acc, _ = m(dev(imgs))
    assert np.array_equal(acc.cpu().numpy(), ref)


@pytest.mark.parametrize("scale", [0.3036, 0.2306, 0.1947, 0.1059, 0.52, 0.0902])
def test_attention_shiftmax_tables_equal_arithmetic(H, scale):
    """ivit_attention_fused_lut (exp_int from the host-built (eps class, distance) tables) == ivit_attention_fused
    (fp32 arithmetic replay) for scales with 1 ... 13 requotient classes, ragged T and saturated scores."""
    tabs = iv.freeze.shiftmax_tables(np.float32(scale))
    assert tabs is not None
    rng = np.random.default_rng(int(scale * 1e4))
    B, Hh, dh = 2, 3, 64
    for T in (197, 50, 577):
        ld = (T + 15) // 16 * 16
        q = dev(rng.integers(-128, 128, (B * Hh, T, dh), dtype=np.int8))
        k = dev(rng.integers(-128, 128, (B * Hh, T, dh), dtype=np.int8))
        vt = np.zeros((B * Hh, dh, ld), np.int8)
        vt[:, :, :T] = rng.integers(-128, 128, (B * Hh, dh, T), dtype=np.int8)
        vt = dev(vt)
        dqk = iv.freeze.dyadic(np.float32(2.2e-4), np.float32(scale))     # scores spread over the whole int8 range
        dpv = iv.freeze.dyadic(np.float32(2.0 ** -15 * 0.1), np.float32(0.05))
        o1 = torch.empty(B, T, Hh * dh, dtype=torch.int8, device="cuda")
        o2 = torch.full_like(o1, 9)
        H.call("ivit_attention_fused", P(q), P(k), P(vt), dyv(dqk), float(scale), dyv(dpv), P(o1), B, Hh, T, dh, ld)
        H.call("ivit_attention_fused_lut", P(q), P(k), P(vt), dyv(dqk), float(scale), P(dev(tabs["aq"])), P(dev(tabs["t"])),
               P(dev(tabs["cls"])), int(tabs["NC"]), int(tabs["t"].size), int(tabs["dmin"]), dyv(dpv), P(o2), B, Hh, T, dh, ld)
        assert np.array_equal(o1.cpu().numpy(), o2.cpu().numpy()), (scale, T)
        assert len(np.unique(o1.cpu().numpy())) > 20
        # round 6: the ROW form of the tables (one gather per score).  The device-built table equals the host restatement
        # (freeze.shiftmax_rowtable) entry for entry; a scale whose lines need more than 64 entries is refused, not truncated
        rt = torch.full((256, 64), -1.0, dtype=torch.float32, device="cuda")
        rt_args = (P(dev(tabs["aq"])), P(dev(tabs["t"])), P(dev(tabs["cls"])), int(tabs["NC"]), int(tabs["t"].size), int(tabs["dmin"]), P(rt))
        if tabs["R"] <= 64:
            H.call("ivit_shiftmax_rowtable", *rt_args)
            assert np.array_equal(rt.cpu().numpy(), iv.freeze.shiftmax_rowtable(tabs))
            o3 = torch.full_like(o1, 9)
            H.call("ivit_attention_fused_rowlut", P(q), P(k), P(vt), dyv(dqk), float(scale), P(rt), int(tabs["dmin"]), dyv(dpv), P(o3), B, Hh, T, dh, ld)
            assert np.array_equal(o1.cpu().numpy(), o3.cpu().numpy()), (scale, T, "row tables")
        else:
            assert iv.freeze.shiftmax_rowtable(tabs) is None
            with pytest.raises(_lib.IvitError, match="64 entries"):
                H.call("ivit_shiftmax_rowtable", *rt_args)
    # the tables are copied in 16-byte pieces: a misaligned exp_t is refused, not mis-read
    shifted = dev(np.concatenate([np.zeros(1, np.float32), tabs["t"]]))
    with pytest.raises(_lib.IvitError, match="16-byte aligned"):
        H.call("ivit_attention_fused_lut", P(q), P(k), P(vt), dyv(dqk), float(scale), P(dev(tabs["aq"])),
               ctypes.c_void_p(shifted.data_ptr() + 4), P(dev(tabs["cls"])), int(tabs["NC"]), int(tabs["t"].size),
               int(tabs["dmin"]), dyv(dpv), P(o2), B, Hh, T, dh, ld)


@pytest.mark.parametrize("scale", [0.06, 0.0431, 0.1947])
def test_window_attention_shiftmax_tables_equal_arithmetic(H, scale):
    """ivit_window_attention_fused_lut (exp_int from freeze.shiftmax_tables in the windows without a shift mask, arithmetic
    under the mask) == ivit_window_attention_fused, with and without the cyclic shift, on grids whose window count makes the
    launcher pick 1, 2 and 4 windows per wavefront (ragged against 8 * wpw)."""
    tabs = iv.freeze.shiftmax_tables(np.float32(scale))
    assert tabs is not None
    rng = np.random.default_rng(int(scale * 1e4))
    aq, et, cl = dev(tabs["aq"]), dev(tabs["t"]), dev(tabs["cls"])
    dqk = iv.freeze.dyadic(np.float32(3.1e-4), np.float32(scale * 0.8))
    da = iv.freeze.dyadic(np.float32(scale * 0.8), np.float32(scale))
    dpv = iv.freeze.dyadic(np.float32(4e-4), np.float32(0.03))
    for B, R, Hh in ((3, 28, 3), (5, 14, 6), (130, 56, 3), (257, 56, 3)):
        qkv = torch.randint(-128, 128, (B, R, R, 3 * Hh * 32), dtype=torch.int8, device="cuda",
                            generator=torch.Generator(device="cuda").manual_seed(B * R))
        relb = dev(rng.integers(-60, 60, (Hh, 49, 49)).astype(np.int16))
        for sh in (0, 3):
            o1 = torch.empty(B, R * R, Hh * 32, dtype=torch.int8, device="cuda")
            o2 = torch.full_like(o1, 9)
            H.call("ivit_window_attention_fused", P(qkv), dyv(dqk), dyv(da), P(relb), float(scale), dyv(dpv), P(o1), B, R, 7, sh, Hh, 32)
            H.call("ivit_window_attention_fused_lut", P(qkv), dyv(dqk), dyv(da), P(relb), float(scale), P(aq), P(et), P(cl),
                   int(tabs["NC"]), int(tabs["t"].size), int(tabs["dmin"]), dyv(dpv), P(o2), B, R, 7, sh, Hh, 32)
            assert torch.equal(o1, o2), (scale, B, R, sh)
        assert len(torch.unique(o1)) > 20


# ---------------------------------------------------------------- persistent pipelined GEMMs (csrc/ivit_gemm3.h)
@pytest.mark.parametrize("M,N,K", [(256, 128, 384), (788, 384, 384), (1000, 1152, 384), (513, 1536, 384), (300, 384, 1536),
                                   (2571, 384, 768), (257, 160, 384), (4099, 256, 1152), (255, 384, 384), (640, 96, 320),
                                   (1300, 768, 768), (600, 1024, 1536), (257, 544, 1152)])
def test_planned_linear_epilogues_vs_oracle(H, M, N, K):
    """ivit_linear_*_planned == oracle linear + requant for the 8-bit, 16-bit and 16-bit + residual epilogues.
    K % 384 == 0 shapes with M >= 256 run gemm_as_kernel (A-stationary for K = 384, streaming rounds above), others the
    launch-per-tile kernels behind the same entry points (and the residual flavour below N = 512); ragged M / N exercise
    the range-checked buffer stores; K >= 768 with N >= 512 the int16 epilogue spread over two rounds."""
    from oracle import oracle as orc
    rng = np.random.default_rng(M + 3 * N + 7 * K)
    x = rng.integers(-128, 128, (M, K), dtype=np.int8)
    w = np.rint(rng.normal(0, 45, (N, K)).clip(-128, 127)).astype(np.int8)
    b = rng.integers(-2 ** 16, 2 ** 16, N).astype(np.int32)
    acc = orc.linear_i8(x, w, b)
    amax = float(np.abs(acc).max())
    s_pre = (10 ** rng.uniform(-6, -4, N)).astype(np.float32)
    s_pre[::5] *= 0.5
    xd, wd, bd = dev(x), dev(w), dev(b)
    for bits in (8, 16):
        s_out = np.float32(amax * float(s_pre.mean()) / 2 ** (bits - 1) * 2.0)
        d = iv.freeze.dyadic(s_pre, s_out)
        dd = dev(d)
        plan = H.linear_plan(P(wd), P(bd), P(dd), N, K)
        out = torch.zeros(M, N, dtype={8: torch.int8, 16: torch.int16}[bits], device="cuda")
        for rep in range(3):      # repeated launches: a wait-count race shows as a run-to-run difference
            H.call("ivit_linear_i8_requant_planned", plan.p, P(xd), bits, P(out), M)
            ref = orc.requant(acc, orc.dyadic(s_pre, s_out), bits)
            assert np.array_equal(out.cpu().numpy().astype(np.int32), ref), (bits, M, N, K, rep)
        plan.close()
    res = rng.integers(-32768, 32768, (M, N)).astype(np.int16)
    s_t = np.float32(amax * float(s_pre.mean()) / 32768 * 2.0)
    d_ch = dev(iv.freeze.dyadic(s_pre, s_t))
    plan = H.linear_plan(P(wd), P(bd), P(d_ch), N, K)
    t = orc.requant(acc, orc.dyadic(s_pre, s_t), 16)
    for s_mid, s_res, s_fin in [(3.1e-5, 7.7e-5, 9.1e-5), (1e-4, 3e-4, 2e-4)]:
        d_main = iv.freeze.dyadic(np.float32(s_mid), np.float32(s_fin))
        d_res = iv.freeze.dyadic(np.float32(s_res), np.float32(s_fin))
        out = torch.zeros(M, N, dtype=torch.int16, device="cuda")
        ref = orc.requant(t, orc.dyadic(np.float32(s_mid), np.float32(s_fin)), 16, res.astype(np.int32),
                          orc.dyadic(np.float32(s_res), np.float32(s_fin)))
        for rep in range(3):
            H.call("ivit_linear_i8_requant_residual_planned", plan.p, P(xd), dyv(d_main), dyv(d_res), P(dev(res)), P(out), M)
            assert np.array_equal(out.cpu().numpy().astype(np.int32), ref), (M, N, K, s_mid, rep)
    plan.close()


@pytest.mark.parametrize("B,T,Hh,dh", [(8, 197, 6, 64), (3, 197, 6, 64), (2, 577, 12, 64), (5, 50, 4, 96)])
def test_planned_qkv_scatter_vs_numpy(H, B, T, Hh, dh):
    """qkv Linear -> QuantAct(8) -> q, k [B,H,T,dh] and v^T [B,H,dh,ldv] through the planned entry point == numpy
    (register-resident epilogue: half-wave exchange + direct 16-byte stores; v^T byte scatter)."""
    from oracle import oracle as orc
    rng = np.random.default_rng(B * 31 + T)
    D = Hh * dh
    M, ld = B * T, (T + 15) // 16 * 16
    x = rng.integers(-128, 128, (M, D), dtype=np.int8)
    w = np.rint(rng.normal(0, 45, (3 * D, D)).clip(-128, 127)).astype(np.int8)
    b = rng.integers(-2 ** 14, 2 ** 14, 3 * D).astype(np.int32)
    acc = orc.linear_i8(x, w, b)
    s_pre = (10 ** rng.uniform(-5.5, -5, 3 * D)).astype(np.float32)
    s_out = np.float32(float(np.abs(acc).max()) * float(s_pre.mean()) / 128 * 1.5)
    d = dev(iv.freeze.dyadic(s_pre, s_out))
    ref = orc.requant(acc, orc.dyadic(s_pre, s_out), 8).reshape(B, T, 3, Hh, dh)
    wd, bd, xd = dev(w), dev(b), dev(x)
    plan = H.linear_plan(P(wd), P(bd), P(d), 3 * D, D)
    q = torch.zeros(B * Hh, T, dh, dtype=torch.int8, device="cuda")
    k = torch.zeros_like(q)
    vt = torch.zeros(B * Hh, dh, ld, dtype=torch.int8, device="cuda")
    H.call("ivit_linear_i8_qkv_planned", plan.p, P(xd), P(q), P(k), P(vt), B, T, Hh, dh, ld)
    assert np.array_equal(q.cpu().numpy().reshape(B, Hh, T, dh), ref[:, :, 0].transpose(0, 2, 1, 3))
    assert np.array_equal(k.cpu().numpy().reshape(B, Hh, T, dh), ref[:, :, 1].transpose(0, 2, 1, 3))
    assert np.array_equal(vt.cpu().numpy().reshape(B, Hh, dh, ld)[..., :T], ref[:, :, 2].transpose(0, 2, 3, 1))
    assert not vt.cpu().numpy().reshape(B, Hh, dh, ld)[..., T:].any()      # the pad stays untouched
    # round 6: ldv = 0 -> v ROW-major [B,H,T,dh] like q and k (one 16-byte store per lane), planned and unplanned entry points;
    # one guard row behind the tensor stays untouched
    for planned in (True, False):
        vr = torch.full((B * Hh * T + 1, dh), 77, dtype=torch.int8, device="cuda")
        q.zero_(); k.zero_()
        if planned:
            H.call("ivit_linear_i8_qkv_planned", plan.p, P(xd), P(q), P(k), P(vr), B, T, Hh, dh, 0)
        else:
            H.call("ivit_linear_i8_qkv", P(xd), P(wd), P(bd), P(d), P(q), P(k), P(vr), B, T, Hh, dh, 0)
        assert np.array_equal(q.cpu().numpy().reshape(B, Hh, T, dh), ref[:, :, 0].transpose(0, 2, 1, 3))
        assert np.array_equal(k.cpu().numpy().reshape(B, Hh, T, dh), ref[:, :, 1].transpose(0, 2, 1, 3))
        assert np.array_equal(vr[:-1].cpu().numpy().reshape(B, Hh, T, dh), ref[:, :, 2].transpose(0, 2, 1, 3)), planned
        assert (vr[-1] == 77).all()
    plan.close()


@pytest.mark.parametrize("B,T", [(1, 197), (3, 197), (9, 50), (37, 197), (256, 197), (300, 197)])
def test_layernorm_qkv_fused_vs_oracle(H, B, T):
    """norm1 + qact1 + attn.qkv of a D = 384 block in one launch (ivit_layernorm_linear_i8_qkv_planned, csrc/ivit_gemm_ws.h;
    vit_quant.py:136-137 + 65-74) and the qkv layer alone on the same kernel (ivit_linear_i8_qkv_planned, ldv = 0, prepared plan):
    q, k, v == the CPU oracle's LayerNorm -> QuantAct(8) -> Linear -> QuantAct(8) for the small batches, == the library's two
    launches on an UNPREPARED plan (gemm_as_kernel) for all of them.  Batches that leave one, several, seven and (B = 300: two
    panels per workgroup) more than seven 32-token tiles per CU; a ragged last tile everywhere; guard rows behind q, k and v."""
    from oracle import oracle as orc
    rng = np.random.default_rng(B * 7 + T)
    D, Hh, dh = 384, 6, 64
    M = B * T
    wln = rng.normal(1.0, 0.4, D).astype(np.float32) * rng.choice([-1.0, 1.0], D).astype(np.float32)
    bln = rng.normal(0.0, 0.5, D).astype(np.float32)
    bias_int, sc = iv.freeze.layernorm_constants(wln, bln)
    s_in, s_out = np.float32(7.3e-4), np.float32(0.031)
    x16 = rng.integers(-26000, 26000, (M, D)).astype(np.int16)
    x16[:, : D // 2] //= 64
    w = np.rint(rng.normal(0, 45, (3 * D, D)).clip(-128, 127)).astype(np.int8)
    b = rng.integers(-2 ** 14, 2 ** 14, 3 * D).astype(np.int32)
    s_pre = (10 ** rng.uniform(-5.5, -5, 3 * D)).astype(np.float32)
    s_q = np.float32(0.02)
    xd, bi_d, sc_d, dln = dev(x16), dev(bias_int), dev(sc), dev(iv.freeze.dyadic(sc, s_out))
    wd, bd, d = dev(w), dev(b), dev(iv.freeze.dyadic(s_pre, s_q))
    plain, prepared = H.linear_plan(P(wd), P(bd), P(d), 3 * D, D), H.linear_plan(P(wd), P(bd), P(d), 3 * D, D)
    H.call("ivit_linear_plan_prepare_ws", prepared.p)
    H.call("ivit_linear_plan_prepare_ws", prepared.p)            # idempotent
    a8 = torch.empty(M, D, dtype=torch.int8, device="cuda")
    H.call("ivit_layernorm_requant", P(xd), M, D, D, float(s_in), P(bi_d), P(sc_d), P(dln), P(a8))
    mk = lambda: [torch.full((B * Hh * T + 1, dh), 77, dtype=torch.int8, device="cuda") for _ in range(3)]
    ref = mk()
    H.call("ivit_linear_i8_qkv_planned", plain.p, P(a8), P(ref[0]), P(ref[1]), P(ref[2]), B, T, Hh, dh, 0)
    if M <= 8000:
        ln8 = orc.requant(orc.layernorm(x16, float(s_in), bias_int, sc), orc.dyadic(sc, s_out), 8)
        assert np.array_equal(a8.cpu().numpy().astype(np.int32), ln8)
        want = orc.requant(orc.linear_i8(ln8.astype(np.int8), w, b), orc.dyadic(s_pre, s_q), 8).reshape(B, T, 3, Hh, dh)
        for i in range(3):
            assert np.array_equal(ref[i][:-1].cpu().numpy().reshape(B, Hh, T, dh), want[:, :, i].transpose(0, 2, 1, 3))
        assert len(np.unique(want)) > 100
    alone, fused = mk(), mk()
    H.call("ivit_linear_i8_qkv_planned", prepared.p, P(a8), P(alone[0]), P(alone[1]), P(alone[2]), B, T, Hh, dh, 0)
    H.call("ivit_layernorm_linear_i8_qkv_planned", prepared.p, P(xd), float(s_in), P(bi_d), P(sc_d), P(dln), P(fused[0]), P(fused[1]), P(fused[2]),
           B, T, Hh, dh)
    for i in range(3):
        assert torch.equal(alone[i], ref[i]), ("qkv on the prepared plan", "qkv"[i], int((alone[i] != ref[i]).sum()))
        assert torch.equal(fused[i], ref[i]), ("LayerNorm + qkv", "qkv"[i], int((fused[i] != ref[i]).sum()))
        assert (ref[i][-1] == 77).all() and (fused[i][-1] == 77).all()
    # the fused launch sized for a share of the CUs (ivit_set_cu_share): more tiles per workgroup, a second panel at the large sizes — same bytes
    for cus in (128, 33):
        shared = mk()
        H.set_cu_share(cus)
        try:
            H.call("ivit_layernorm_linear_i8_qkv_planned", prepared.p, P(xd), float(s_in), P(bi_d), P(sc_d), P(dln), P(shared[0]), P(shared[1]), P(shared[2]),
                   B, T, Hh, dh)
        finally:
            H.set_cu_share(0)
        for i in range(3):
            assert torch.equal(shared[i], ref[i]), (cus, "qkv"[i], int((shared[i] != ref[i]).sum()))
    # a plan that was not prepared, a head dim the kernel is not built for: refused, nothing launched
    for pl, hh, dd in ((plain, Hh, dh), (prepared, 12, 32)):
        with pytest.raises(_lib.IvitError, match="prepare_ws"):
            H.call("ivit_layernorm_linear_i8_qkv_planned", pl.p, P(xd), float(s_in), P(bi_d), P(sc_d), P(dln), P(fused[0]), P(fused[1]), P(fused[2]),
                   B, T, hh, dd)
    plain.close(); prepared.close()


@pytest.mark.parametrize("B,C,HW,D", [(1, 3, 224, 384), (5, 3, 224, 384), (3, 3, 64, 192), (2, 1, 96, 768), (70, 3, 224, 384)])
def test_patch_embed_one_launch_equals_three(H, B, C, HW, D):
    """PatchEmbed -> QuantAct(16) -> class token + position embedding -> QuantAct(16) (layers_quant.py:184-196, vit_quant.py:255-265) as ONE
    GEMM launch that gathers its rows from the images (ivit_patch_embed) == ivit_im2col_patch + ivit_linear_i8_requant(16) +
    ivit_embed_finish (each pinned against the oracle elsewhere), bit for bit, guard row behind the output; the form is refused for
    8 x 8 patches and for multipliers outside the fast range."""
    rng = np.random.default_rng(B * 131 + HW + D)
    P16, g = 16, HW // 16
    np_, K, T = g * g, C * 256, g * g + 1
    img = dev(rng.integers(-128, 128, (B, C, HW, HW), dtype=np.int8))
    w = dev(np.rint(rng.normal(0, 40, (D, K)).clip(-128, 127)).astype(np.int8))
    b = dev(rng.integers(-2 ** 14, 2 ** 14, D).astype(np.int32))
    d = dev(iv.freeze.dyadic((10 ** rng.uniform(-5.5, -5, D)).astype(np.float32), np.float32(2e-4)))
    z_cls = dev(rng.integers(-10 ** 6, 10 ** 6, D).astype(np.int32))
    pos = dev(rng.integers(-20000, 20000, (T, D)).astype(np.int16))
    dx, dp = iv.freeze.dyadic(np.float32(2e-4), np.float32(7e-4)), iv.freeze.dyadic(np.float32(5e-4), np.float32(7e-4))
    rows = torch.empty(B * np_, K, dtype=torch.int8, device="cuda")
    p16 = torch.empty(B * np_, D, dtype=torch.int16, device="cuda")
    want = torch.full((B * T + 1, D), 77, dtype=torch.int16, device="cuda")
    got = torch.full((B * T + 1, D), 77, dtype=torch.int16, device="cuda")
    H.call("ivit_im2col_patch", P(img), B, C, HW, HW, P16, P(rows))
    H.call("ivit_linear_i8_requant", P(rows), P(w), P(b), P(d), 16, P(p16), B * np_, D, K)
    H.call("ivit_embed_finish", P(p16), P(z_cls), P(pos), dyv(dx), dyv(dp), P(want), B, T, D)
    H.call("ivit_patch_embed", P(img), B, C, HW, HW, P16, P(w), P(b), P(d), P(z_cls), P(pos), dyv(dx), dyv(dp), P(got), D)
    assert torch.equal(got, want), int((got != want).sum())
    assert (got[-1] == 77).all() and len(torch.unique(want)) > 1000
    with pytest.raises(_lib.IvitError, match="16 x 16"):
        H.call("ivit_patch_embed", P(img), B, C, HW, HW, 8, P(w), P(b), P(d), P(z_cls), P(pos), dyv(dx), dyv(dp), P(got), D)
    with pytest.raises(_lib.IvitError, match="16 x 16"):
        H.call("ivit_patch_embed", P(img), B, C, HW, HW, P16, P(w), P(b), P(d), P(z_cls), P(pos), _lib.Dyadic(1024.0, 1.0), dyv(dp), P(got), D)


@pytest.mark.parametrize("M,N", [(1, 1152), (196, 1152), (6000, 1152), (50176, 1152), (3000, 64), (3000, 1536)])
def test_layernorm_linear_plain_fused_vs_oracle(H, M, N):
    """IntLayerNorm -> QuantAct(8) -> QuantLinear -> QuantAct(8) with a plain [M, N] output in one launch
    (ivit_layernorm_linear_i8_requant_planned: norm1 + attn.qkv of a Swin C = 384 block, swin_quant.py:256-258) and
    ivit_linear_i8_requant_planned(bits = 8) on a prepared plan: == the oracle for the small shapes, == the two launches on an
    unprepared plan for all; guard rows."""
    from oracle import oracle as orc
    rng = np.random.default_rng(M * 3 + N)
    D = 384
    wln = rng.normal(1.0, 0.4, D).astype(np.float32) * rng.choice([-1.0, 1.0], D).astype(np.float32)
    bias_int, sc = iv.freeze.layernorm_constants(wln, rng.normal(0.0, 0.5, D).astype(np.float32))
    s_in, s_out = np.float32(7.3e-4), np.float32(0.031)
    x16 = rng.integers(-26000, 26000, (M, D)).astype(np.int16)
    x16[:, : D // 2] //= 64
    w = np.rint(rng.normal(0, 45, (N, D)).clip(-128, 127)).astype(np.int8)
    b = rng.integers(-2 ** 14, 2 ** 14, N).astype(np.int32)
    s_pre, s_q = (10 ** rng.uniform(-5.5, -5, N)).astype(np.float32), np.float32(0.02)
    xd, bi_d, sc_d, dln = dev(x16), dev(bias_int), dev(sc), dev(iv.freeze.dyadic(sc, s_out))
    wd, bd, d = dev(w), dev(b), dev(iv.freeze.dyadic(s_pre, s_q))
    plain, prepared = H.linear_plan(P(wd), P(bd), P(d), N, D), H.linear_plan(P(wd), P(bd), P(d), N, D)
    H.call("ivit_linear_plan_prepare_ws", prepared.p)
    a8 = torch.empty(M, D, dtype=torch.int8, device="cuda")
    H.call("ivit_layernorm_requant", P(xd), M, D, D, float(s_in), P(bi_d), P(sc_d), P(dln), P(a8))
    mk = lambda: torch.full((M + 1, N), 77, dtype=torch.int8, device="cuda")
    ref, alone, fused = mk(), mk(), mk()
    H.call("ivit_linear_i8_requant_planned", plain.p, P(a8), 8, P(ref), M)
    H.call("ivit_linear_i8_requant_planned", prepared.p, P(a8), 8, P(alone), M)
    H.call("ivit_layernorm_linear_i8_requant_planned", prepared.p, P(xd), float(s_in), P(bi_d), P(sc_d), P(dln), P(fused), M)
    assert torch.equal(alone, ref) and torch.equal(fused, ref), (int((alone != ref).sum()), int((fused != ref).sum()))
    assert (ref[-1] == 77).all()
    if M * N <= 8_000_000:
        ln8 = orc.requant(orc.layernorm(x16, float(s_in), bias_int, sc), orc.dyadic(sc, s_out), 8)
        want = orc.requant(orc.linear_i8(ln8.astype(np.int8), w, b), orc.dyadic(s_pre, s_q), 8)
        assert np.array_equal(ref[:-1].cpu().numpy().astype(np.int32), want) and len(np.unique(want)) > 50
    with pytest.raises(_lib.IvitError, match="prepare_ws"):
        H.call("ivit_layernorm_linear_i8_requant_planned", plain.p, P(xd), float(s_in), P(bi_d), P(sc_d), P(dln), P(fused), M)
    plain.close(); prepared.close()


@pytest.mark.parametrize("M,N", [(1, 384), (197, 384), (591, 384), (7000, 384), (50432, 384), (60000, 384), (1000, 128), (1000, 1536)])
def test_residual_linear_on_prepared_plan_vs_oracle(H, M, N):
    """attn.proj + qact2 with the identity branch (vit_quant.py:137-138, quant_utils.py:238-244) of a K = 384 layer on
    gemm_ws_qkv_kernel<.., EPI_RES16> (ivit_linear_plan_prepare_ws + ivit_linear_i8_requant_residual_planned): == the CPU oracle
    for the small shapes, == the same call on an unprepared plan for all; ragged last tiles, one to more than seven 32-token
    tiles per CU (two panels), 2 / 6 / 24 channel slabs, a guard row behind the output."""
    from oracle import oracle as orc
    rng = np.random.default_rng(M + N)
    K = 384
    x = rng.integers(-128, 128, (M, K), dtype=np.int8)
    w = np.rint(rng.normal(0, 45, (N, K)).clip(-128, 127)).astype(np.int8)
    b = rng.integers(-2 ** 14, 2 ** 14, N).astype(np.int32)
    s_pre = (10 ** rng.uniform(-5.5, -5, N)).astype(np.float32)
    s_mid, s_res, s_out = np.float32(2e-4), np.float32(6.9e-4), np.float32(7.3e-4)
    res = rng.integers(-30000, 30000, (M, N)).astype(np.int16)
    xd, wd, bd, rd, d = dev(x), dev(w), dev(b), dev(res), dev(iv.freeze.dyadic(s_pre, s_mid))
    dm, dr = iv.freeze.dyadic(s_mid, s_out), iv.freeze.dyadic(s_res, s_out)
    plain, prepared = H.linear_plan(P(wd), P(bd), P(d), N, K), H.linear_plan(P(wd), P(bd), P(d), N, K)
    H.call("ivit_linear_plan_prepare_ws", prepared.p)
    outs = []
    for pl in (plain, prepared):
        o = torch.full((M + 1, N), 77, dtype=torch.int16, device="cuda")
        H.call("ivit_linear_i8_requant_residual_planned", pl.p, P(xd), dyv(dm), dyv(dr), P(rd), P(o), M)
        assert (o[-1] == 77).all()
        outs.append(o[:-1])
    assert torch.equal(outs[0], outs[1]), int((outs[0] != outs[1]).sum())
    if M * N <= 3_000_000:
        t16 = orc.requant(orc.linear_i8(x, w, b), orc.dyadic(s_pre, s_mid), 16)
        want = orc.requant(t16, orc.dyadic(s_mid, s_out), 16, res.astype(np.int32), orc.dyadic(s_res, s_out))
        assert np.array_equal(outs[1].cpu().numpy().astype(np.int32), want)
        assert len(np.unique(want)) > min(1000, M * N // 4)
    # norm2 + qact3 in the tail of the same launch (ivit_linear_i8_requant_residual_layernorm_planned): the 16-bit rows and
    # ivit_layernorm_requant of them; refused for anything but a prepared 384 x 384 plan
    wln = rng.normal(1.0, 0.4, K).astype(np.float32) * rng.choice([-1.0, 1.0], K).astype(np.float32)
    bias_int, sc = iv.freeze.layernorm_constants(wln, rng.normal(0.0, 0.5, K).astype(np.float32))
    bi_d, sc_d, dln = dev(bias_int), dev(sc), dev(iv.freeze.dyadic(sc, np.float32(0.031)))
    o16 = torch.full((M + 1, N), 77, dtype=torch.int16, device="cuda")
    o8 = torch.full((M + 1, N), 77, dtype=torch.int8, device="cuda")
    args = (P(xd), dyv(dm), dyv(dr), P(rd), P(o16), M, float(s_out), P(bi_d), P(sc_d), P(dln), P(o8))
    if N == 384:
        H.call("ivit_linear_i8_requant_residual_layernorm_planned", prepared.p, *args)
        want8 = torch.empty(M, N, dtype=torch.int8, device="cuda")
        H.call("ivit_layernorm_requant", P(outs[0]), M, N, N, float(s_out), P(bi_d), P(sc_d), P(dln), P(want8))
        assert torch.equal(o16[:-1], outs[0]) and torch.equal(o8[:-1], want8), (int((o16[:-1] != outs[0]).sum()), int((o8[:-1] != want8).sum()))
        assert (o16[-1] == 77).all() and (o8[-1] == 77).all() and len(torch.unique(want8)) > min(100, M)
    for pl in ((plain,) if N == 384 else (plain, prepared)):
        with pytest.raises(_lib.IvitError, match="prepare_ws"):
            H.call("ivit_linear_i8_requant_residual_layernorm_planned", pl.p, *args)
    plain.close(); prepared.close()


def test_linear_plan_bounds_and_fallback(H):
    """the plan proves the pipelined kernel's exactness bounds per channel; a layer outside them (|z*c| may reach 2^31)
    must be routed to the saturating launch-per-tile kernel and still match the oracle."""
    from oracle import oracle as orc
    rng = np.random.default_rng(99)
    M, N, K = 512, 256, 384
    x = rng.integers(-128, 128, (M, K), dtype=np.int8)
    w = rng.integers(-128, 128, (N, K), dtype=np.int8)
    b = rng.integers(-2 ** 10, 2 ** 10, N).astype(np.int32)
    acc = orc.linear_i8(x, w, b)
    xd, wd, bd = dev(x), dev(w), dev(b)
    s_small = np.full(N, 1e-5, np.float32)
    p_ok = H.linear_plan(P(wd), P(bd), P(dev(iv.freeze.dyadic(s_small, np.float32(1.0)))), N, K)
    assert p_ok.pipelined_ok and p_ok.single_fma_ok
    s_big = s_small.copy()
    s_big[7] = 3.0e4                      # |z*c| up to ~2^37 on one channel
    d_big = iv.freeze.dyadic(s_big, np.float32(1.0))
    p_bad = H.linear_plan(P(wd), P(bd), P(dev(d_big)), N, K)
    assert not p_bad.pipelined_ok
    out = torch.zeros(M, N, dtype=torch.int8, device="cuda")
    H.call("ivit_linear_i8_requant_planned", p_bad.p, P(xd), 8, P(out), M)
    assert np.array_equal(out.cpu().numpy().astype(np.int32), orc.requant(acc, orc.dyadic(s_big, np.float32(1.0)), 8))
    # a dense +-127 weight row with K = 1536 pushes 128 * sum|w| * m past 2^53: the cheap one-FMA bound fails and the plan
    # decides channel by channel at the rounding boundaries (linear_plan_fma_kernel, round 4); whichever form runs, the
    # results are the oracle's
    K2 = 1536
    w2 = np.full((N, K2), 127, np.int8)
    w2[::2] *= -1
    x2 = rng.integers(-128, 128, (M, K2), dtype=np.int8)
    d2 = dev(iv.freeze.dyadic(np.full(N, 1e-6, np.float32), np.float32(0.05)))
    p2 = H.linear_plan(P(dev(w2)), P(bd), P(d2), N, K2)
    assert p2.pipelined_ok
    # which form: the one-FMA requant exactly when NO z within the plan's bound 128 * sum|w| + |bias| of any channel rounds
    # differently once and twice (tests/two_roundings.py enumerates those z exactly; tests/test_requant_two_roundings_gpu.py
    # pins the decision where such a z exists).  Here (m = 1407374859, e = 46) there is none: the proof must succeed
    import two_roundings as tr
    m2, r2 = iv.freeze.dyadic(np.float32(1e-6), np.float32(0.05))[0]
    zs = tr.differing(int(m2), int(round(-np.log2(r2))), 128 * 127 * K2 + int(np.abs(b).max()))
    assert p2.single_fma_ok == (not zs) and p2.single_fma_ok, zs
    out2 =torch.zeros(M, N, dtype=torch.int8, device="cuda")
    H.call("ivit_linear_i8_requant_planned", p2.p, P(dev(x2)), 8, P(out2), M)
    ref2 = orc.requant(orc.linear_i8(x2, w2, b), orc.dyadic(np.full(N, 1e-6, np.float32), np.float32(0.05)), 8)
    assert np.array_equal(out2.cpu().numpy().astype(np.int32), ref2)
    for pl in (p_ok, p_bad, p2):
        pl.close()


# ---------------------------------------------------------------- fake-quant fp32 convention (SURVEY.md §8b "accepting either")
def _micro_model(g):
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    m = iv.VisionTransformer(img_size=cfg.img_size, patch_size=cfg.patch_size, num_classes=cfg.num_classes,
                             embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=4)
    m.load_float_weights(iv.make_vit_weights(cfg, int(g["seed"]))).load_act_scales(golden_scales(g))
    iv.freeze_model(m)
    return cfg, m


@pytest.mark.parametrize("fname", ["micro_vit_b2.npz", "micro_vit2h_b3.npz"])
def test_fake_quant_tensors_through_operator_surface_golden(fname):
    """every operator fed the reference's OWN tensor convention — fp32 X = fl(Q*s) with its scale — returns the fp32
    tensor the reference returns: rne(Y / s_out) equals the golden integers at every one of the operator sites, the
    `attn * self.scale` step of Attention.forward (vit_quant.py:72-73) included, and the logits come back as fp32."""
    g = load_golden(fname)
    cfg, m = _micro_model(g)
    m.fake_quant = True
    seen = {}

    def hook(name):
        def f(mod, inp, out):
            y, s = out
            assert y.is_floating_point() and type(y) is torch.Tensor, name     # plain fp32, not the IntValued marker
            sv = torch.as_tensor(np.asarray(s.detach().cpu().numpy() if isinstance(s, torch.Tensor) else s, np.float32))
            if sv.dim() != y.dim():                  # scalar, or per-channel on the last dim
                sv = sv.reshape(-1)
                sv = sv if sv.numel() == 1 else sv.reshape([1] * (y.dim() - 1) + [-1])
            seen[name] = torch.round(y.cpu() / sv).numpy()
        return f
    for name, mod in m.named_modules():
        if f"site/{name}" in g.files:
            mod.register_forward_hook(hook(name))
    imgs = iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"]))
    s_in = golden_scales(g)["qact_input"]
    x = dev((imgs.astype(np.float32) * np.float32(s_in)).astype(np.float32))       # the reference's input: q * s
    with torch.no_grad():
        logits, s_head = m(x)
    assert logits.dtype == torch.float32
    acc = torch.round(logits.cpu() / torch.as_tensor(np.asarray(s_head, np.float32))).numpy().astype(np.int64)
    assert np.array_equal(acc, g["logits_int"])
    checked = 0
    for name, got in seen.items():
        ref = g[f"site/{name}"].astype(np.float64)
        if name.endswith("attn.matmul_2"):
            continue      # the reference's own fp32 bmm of non-integers is off by +-1 there
        if got.ndim == 4 and ref.ndim == 3:        # conv layout [B, C, H, W] vs the fixture's flatten(2).transpose(1, 2)
            got = got.reshape(got.shape[0], got.shape[1], -1).transpose(0, 2, 1)
        if name == "norm" and got.ndim == 3 and ref.ndim == 2:
            got = got[:, 0]                         # the fixture keeps the class-token rows of the final norm
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        assert np.array_equal(got.astype(np.float64), ref), name
        checked += 1
    assert checked >= 40


def test_swin_fake_quant_tensors_with_float_mask_golden():
    """config 4 through the reference's OWN tensor convention.  SwinTransformer(fake_quant=True) runs the
    reference's statements on fp32 X = fl(Q*s) tensors — including `attn + mask` with the float -100 mask added to the
    fake-quant logits before Shiftmax (swin_quant.py:151-156), which IntSoftmax takes as the integer-domain side input it
    is — and every operator site of the micro-Swin fixture (shifted windows included) returns the reference's integers."""
    from ivit_amd.swin_quant import SwinTransformer
    g = load_golden("micro_swin_b2.npz")
    cfg = iv.SWIN_CONFIGS[str(g["cfg_name"])]
    m = SwinTransformer(img_size=cfg.img_size, patch_size=cfg.patch_size, num_classes=cfg.num_classes,
                        embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads,
                        window_size=cfg.window_size, mlp_ratio=cfg.mlp_ratio)
    m.load_float_weights(iv.make_swin_weights(cfg, int(g["seed"]))).load_act_scales(golden_scales(g))
    iv.freeze_model(m)
    m.fake_quant = True
    assert any(blk.attn_mask is not None for layer in m.layers for blk in layer.blocks)      # shifted windows exist
    seen = {}

    def hook(name):
        def f(mod, inp, out):
            y, s = out
            if name.endswith("qact_table"):       # a quantised PARAMETER (no pre-scale): the integers themselves
                seen[name] = y.cpu().numpy().astype(np.float64)
                return
            assert y.is_floating_point() and type(y) is torch.Tensor, name
            sv = torch.as_tensor(np.asarray(s.detach().cpu().numpy() if isinstance(s, torch.Tensor) else s, np.float32))
            if sv.dim() != y.dim():
                sv = sv.reshape(-1)
                sv = sv if sv.numel() == 1 else sv.reshape([1] * (y.dim() - 1) + [-1])
            seen[name] = torch.round(y.cpu() / sv).numpy()
        return f
    for name, mod in m.named_modules():
        if f"site/{name}" in g.files:
            mod.register_forward_hook(hook(name))
    imgs = iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"]))
    s_in = golden_scales(g)["qact_input"]
    x = dev((imgs.astype(np.float32) * np.float32(s_in)).astype(np.float32))
    with torch.no_grad():
        logits, s_head = m(x)
    assert logits.dtype == torch.float32
    acc = torch.round(logits.cpu() / torch.as_tensor(np.asarray(s_head, np.float32))).numpy().astype(np.int64)
    assert np.array_equal(acc, g["logits_int"])
    checked = masked_sites = 0
    for name, got in seen.items():
        ref = g[f"site/{name}"].astype(np.float64)
        if name.endswith("attn.matmul_2"):
            continue      # the reference's own fp32 bmm of non-integers is off by +-1 there
        if got.ndim == 4 and ref.ndim == 3 and name == "patch_embed.proj":
            got = got.reshape(got.shape[0], got.shape[1], -1).transpose(0, 2, 1)
        assert got.size == ref.size, (name, got.shape, ref.shape)
        assert np.array_equal(got.reshape(ref.shape).astype(np.float64), ref), name
        checked += 1
        masked_sites += name.endswith("log_int_softmax")
    assert checked >= 90 and masked_sites >= 2


def test_intsoftmax_recovers_float_masked_logits(H):
    """IntSoftmax on fp32 logits with the reference's float mask already added (-100.0 on the masked entries) == the
    integer call with the mask passed as a side input; logits that are off the grid for any other reason are refused."""
    rng = np.random.default_rng(8)
    s = np.float32(0.0473)
    q = rng.integers(-128, 128, (6, 3, 49, 49)).astype(np.int8)
    mask = np.where(rng.random((2, 49, 49)) < 0.3, np.float32(-100.0), np.float32(0.0)).astype(np.float32)
    sm = iv.IntSoftmax(8)
    ref, s_out = sm(dev(q), s, mask=dev(mask), num_heads=3)
    X = (q.astype(np.float32) * s).astype(np.float32).reshape(3, 2, 3, 49, 49) + mask[None, :, None]
    got, s_out2 = sm(dev(X.reshape(6, 3, 49, 49).astype(np.float32)), s)
    assert got.is_floating_point()
    assert np.array_equal(torch.round(got.cpu() / s_out2).numpy().astype(np.int64), ref.cpu().numpy().astype(np.int64))
    bad = X.reshape(6, 3, 49, 49).copy()
    bad[0, 0, 0, 0] += np.float32(0.4) * s            # off the grid although no mask value explains it
    with pytest.raises(ValueError):
        sm(dev(bad.astype(np.float32)), s)


def test_fake_quant_rejects_off_grid_tensors(H):
    """a float that is not integer * scale (e.g. logits with a -100.0 mask added) is refused, never rounded silently"""
    sm = iv.IntSoftmax(16)
    x = torch.randn(2, 4, 8, device="cuda")
    with pytest.raises(ValueError):
        sm(x, np.float32(0.05))
    lin = iv.QuantLinear(64, 32)
    with pytest.raises(ValueError):
        lin(torch.full((4, 64), 1000.0, device="cuda"), np.float32(1.0))       # outside int8 for this scale


def test_reloaded_weights_requantise(H):
    """the frozen-integer cache of QuantLinear / IntLayerNorm follows the float parameters — loading new
    weights into a model that has already run must change the integers it computes with."""
    from oracle import oracle as orc
    rng = np.random.default_rng(3)
    lin = iv.QuantLinear(64, 32).cuda()
    x = dev(rng.integers(-128, 128, (8, 64), dtype=np.int8))
    outs = []
    for seed in (1, 2):
        w = np.random.default_rng(seed).normal(0, 0.05, (32, 64)).astype(np.float32)
        b = np.random.default_rng(seed + 10).normal(0, 0.1, 32).astype(np.float32)
        lin.load_state_dict({"weight": torch.from_numpy(w), "bias": torch.from_numpy(b)}, strict=False)
        acc, s = lin(x, np.float32(0.02))
        w_int, s_w = iv.freeze.quantize_weight(w)
        b_int, _ = iv.freeze.quantize_bias(b, s_w, np.float32(0.02))
        assert np.array_equal(acc.cpu().numpy(), orc.linear_i8(x.cpu().numpy(), w_int, b_int)), seed
        outs.append(acc.cpu().numpy())
    assert not np.array_equal(outs[0], outs[1])
    ln = iv.IntLayerNorm(64).cuda()
    xi = dev(rng.integers(-3000, 3000, (2, 5, 64)).astype(np.int16))
    z1, _ = ln(xi, np.float32(0.01))
    with torch.no_grad():
        ln.weight.copy_(torch.linspace(0.5, 2.0, 64))
    z2, _ = ln(xi, np.float32(0.01))
    assert not torch.equal(z1, z2)


def test_ragged_slices_head_dim_32():
    """uneven slices (5 images over 3 streams) on the unfused-attention path (head dim 32) — every slice
    runs on the largest slice's buffer layout, whose pads ivit_vit_workspace_init zeroed."""
    from oracle import oracle as orc
    cfg = iv.ViTConfig("ragged32", img_size=24, patch_size=8, num_classes=7, embed_dim=64, depth=2, num_heads=2)
    assert cfg.head_dim == 32
    w = iv.make_vit_weights(cfg, seed=5)
    m = iv.VisionTransformer(img_size=24, patch_size=8, num_classes=7, embed_dim=64, depth=2, num_heads=2, mlp_ratio=4)
    m.load_float_weights(w)
    with torch.no_grad():
        m(dev(iv.make_calibration_batch(cfg, 3, seed=17)))
    iv.freeze_model(m)
    sc = {k: v for k, v in m.act_scales().items() if v > 0}
    eng = m.compile()
    imgs = iv.make_images_int8(cfg, 5, seed=23)
    ref, _ = orc.OracleViT(cfg, w, sc).forward(imgs)
    for ns in (3, 2, 1):
        got = eng.forward(dev(imgs), nslices=ns, copy=True).cpu().numpy()
        assert np.array_equal(got, ref), ns
    a = eng.forward(dev(imgs), nslices=1, copy=True)
    b = eng.forward(dev(iv.make_images_int8(cfg, 5, seed=24)), nslices=1)
    assert not torch.equal(a, b)          # copy=True: `a` survived the second forward


def test_constants_upload_and_rccl_broadcast(H):
    """the C-ABI path a C host uses to distribute the packed integer constants: ivit_constants_upload (host -> device)
    and ivit_constants_broadcast (ncclBroadcast over a caller-supplied RCCL communicator).  One GPU here: a 1-rank
    communicator made with librccl directly (ncclGetUniqueId + ncclCommInitRank) — the broadcast must leave rank 0's
    bytes intact and the uploaded blob must drive the native runner to the golden logits."""
    import ctypes
    from ivit_amd.engine import ViTEngine, pack_constants
    g = load_golden("micro_vit_b2.npz")
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    consts, f32 = iv.freeze.freeze_vit(cfg, iv.make_vit_weights(cfg, int(g["seed"])), golden_scales(g))
    blob, table = pack_constants(consts)
    dblob = torch.zeros(blob.size, dtype=torch.uint8, device="cuda")
    H.call("ivit_constants_upload", blob.ctypes.data_as(_P), blob.size, P(dblob))
    rccl = ctypes.CDLL("librccl.so")

    class UID(ctypes.Structure):
        _fields_ = [("b", ctypes.c_char * 128)]
    uid, comm = UID(), ctypes.c_void_p()
    assert rccl.ncclGetUniqueId(ctypes.byref(uid)) == 0
    rccl.ncclCommInitRank.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, UID, ctypes.c_int]
    assert rccl.ncclCommInitRank(ctypes.byref(comm), 1, uid, 0) == 0
    H.call("ivit_constants_broadcast", P(dblob), blob.size, 0, comm)
    torch.cuda.synchronize()
    assert np.array_equal(dblob.cpu().numpy(), blob)
    rccl.ncclCommDestroy.argtypes = [ctypes.c_void_p]
    rccl.ncclCommDestroy(comm)
    eng = ViTEngine(cfg, None, f32, blob=dblob, table=table)
    imgs = iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"]))
    assert np.array_equal(eng.forward(dev(imgs)).cpu().numpy(), g["logits_int"])


# ---------------------------------------------------------------- full-size configs, model zoo, Swin checkpoints
@pytest.mark.parametrize("fname,B", [("deit_base_b2.npz", 64), ("vit_base_384_b1.npz", 128)])
def test_full_size_batch_properties_vit_configs(fname, B):
    """BASELINE configs 3 and 5 at the per-GPU batch they name (DeiT-B 512 / 8 = 64, ViT-B@384 1024 / 8 = 128): large-M
    code paths (grid caps, 64-bit offsets, XCD maps, the pipelined GEMMs' multi-round K = 768 / 3072) under the same
    size-independent properties as DeiT-S — golden prefix, permutation equivariance, duplicates, slices, hipGraph."""
    g = load_golden(fname)
    cfg, w, eng = _engine_for(g)
    gb = int(g["batch"])
    imgs = np.concatenate([iv.make_images_int8(cfg, gb, int(g["images_seed"])), iv.make_images_int8(cfg, B - gb, seed=11)])
    imgs[B - gb:] = imgs[:gb]                                   # duplicates at the far end of the batch
    d = dev(imgs)
    ref = eng.forward(d, copy=True).cpu().numpy()
    assert np.array_equal(ref[:gb], g["logits_int"])
    assert np.array_equal(ref[B - gb:], ref[:gb])
    perm = np.random.default_rng(5).permutation(B)
    assert np.array_equal(eng.forward(dev(imgs[perm])).cpu().numpy(), ref[perm])
    assert np.array_equal(eng.forward(d, nslices=2).cpu().numpy(), ref)
    rep = eng.capture(d, 2)
    out = rep()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref)
    # DeiT-B: 32 of the 60 non-golden, non-duplicate images; ViT-B@384 (13x the work per image): 8
    _oracle_sample_check(cfg, w, golden_scales(g), imgs[:B - gb], ref, 32 if B == 64 else 8, first_free=gb)


def test_full_size_batch_properties_swin_tiny_b256():
    """BASELINE config 4 at full size (Swin-T, 256 images) through the native Swin runner."""
    from ivit_amd.swin_engine import SwinEngine
    g = load_golden("swin_tiny_b1.npz")
    cfg = iv.SWIN_CONFIGS[str(g["cfg_name"])]
    eng = SwinEngine(cfg, iv.make_swin_weights(cfg, int(g["seed"])), golden_scales(g))
    B = 256
    imgs = np.concatenate([iv.make_images_int8(cfg, 1, int(g["images_seed"])), iv.make_images_int8(cfg, B - 1, seed=11)])
    imgs[255] = imgs[0]
    d = dev(imgs)
    ref = eng.forward(d).clone().cpu().numpy()
    assert np.array_equal(ref[:1], g["logits_int"])
    assert np.array_equal(ref[255], ref[0])
    perm = np.random.default_rng(7).permutation(B)
    assert np.array_equal(eng.forward(dev(imgs[perm])).cpu().numpy(), ref[perm])
    assert np.array_equal(eng.forward(d, nslices=4).cpu().numpy(), ref)
    rep = eng.capture(d, 4)
    out = rep()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref)
    _oracle_sample_check(cfg, iv.make_swin_weights(cfg, int(g["seed"])), golden_scales(g), imgs[:255], ref, 8, first_free=1, swin=True)


def test_model_zoo_vit_large_golden():
    """vit_large_patch16_224 (D = 1024, 24 blocks, 16 heads; vit_quant.py:365-381) through the native
    runner and the per-operator path == the reference's int32 logits."""
    g = load_golden("vit_large_b1.npz")
    cfg, w, eng = _engine_for(g)
    imgs = dev(iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"])))
    assert np.array_equal(eng.forward(imgs).cpu().numpy(), g["logits_int"])
    assert np.array_equal(eng.forward_ops(imgs).cpu().numpy(), g["logits_int"])
    m = iv.vit_large_patch16_224()
    assert (m.cfg.embed_dim, m.cfg.depth, m.cfg.num_heads) == (cfg.embed_dim, cfg.depth, cfg.num_heads)


def test_model_zoo_swin_small_golden():
    """swin_small_patch4_window7_224 (depths 2/2/18/2; swin_quant.py:588-606): the fused SwinEngine
    (C = 96 stage-0 fused Mlp, window attention) and the reference-shaped operator chain == the reference's logits."""
    from ivit_amd.swin_engine import SwinEngine
    from ivit_amd.swin_quant import SwinTransformer
    g = load_golden("swin_small_b1.npz")
    cfg = iv.SWIN_CONFIGS[str(g["cfg_name"])]
    w = iv.make_swin_weights(cfg, int(g["seed"]))
    imgs = iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"]))
    eng = SwinEngine(cfg, w, golden_scales(g))
    assert np.array_equal(eng.forward(dev(imgs)).cpu().numpy(), g["logits_int"])
    assert np.array_equal(eng.forward(dev(np.concatenate([imgs, imgs, imgs])), nslices=3).cpu().numpy(),
                          np.concatenate([g["logits_int"]] * 3))
    m = SwinTransformer(img_size=cfg.img_size, patch_size=cfg.patch_size, num_classes=cfg.num_classes,
                        embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads,
                        window_size=cfg.window_size, mlp_ratio=cfg.mlp_ratio)
    m.load_float_weights(w).load_act_scales(golden_scales(g))
    iv.freeze_model(m)
    with torch.no_grad():
        acc, _ = m(dev(imgs))
    assert np.array_equal(acc.cpu().numpy(), g["logits_int"])


def test_model_zoo_swin_base_golden():
    """swin_base_patch4_window7_224 (embed 128, heads 4/8/16/32, depths 2/2/18/2; swin_quant.py:609-627) — channel
    counts 128 / 256 / 512 / 1024 (and 2048 in the last PatchMerging) that no other fixture exercises: the fused SwinEngine,
    a sliced forward and the reference-shaped operator chain built by the FACTORY == the reference's int32 logits."""
    from ivit_amd.swin_engine import SwinEngine
    g = load_golden("swin_base_b1.npz")
    cfg = iv.SWIN_CONFIGS[str(g["cfg_name"])]
    assert (cfg.embed_dim, tuple(cfg.num_heads), tuple(cfg.depths)) == (128, (4, 8, 16, 32), (2, 2, 18, 2))
    w = iv.make_swin_weights(cfg, int(g["seed"]))
    imgs = iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"]))
    eng = SwinEngine(cfg, w, golden_scales(g))
    assert np.array_equal(eng.forward(dev(imgs)).cpu().numpy(), g["logits_int"])
    assert np.array_equal(eng.forward(dev(np.concatenate([imgs, imgs])), nslices=2).cpu().numpy(), np.concatenate([g["logits_int"]] * 2))
    m = iv.swin_base_patch4_window7_224()
    m.load_float_weights(w).load_act_scales(golden_scales(g))
    iv.freeze_model(m)
    with torch.no_grad():
        acc, scale = m(dev(imgs))
    assert np.array_equal(acc.cpu().numpy(), g["logits_int"])
    assert np.array_equal(scale.numpy(), g["logits_scale"])


def test_imported_reference_swin_state_dict_runs_to_golden_logits():
    """checkpoint importer on a SWIN state dict (the reference's own post-forward `state_dict()`, buffers stored as a
    fixture): -> operator chain and fused SwinEngine -> the reference's logits."""
    from ivit_amd import checkpoint as ck
    from ivit_amd.swin_quant import SwinTransformer
    from ivit_amd.swin_engine import SwinEngine
    f = load_golden("micro_swin_state_dict.npz")
    g = load_golden("micro_swin_b2.npz")
    cfg = iv.SWIN_CONFIGS[str(f["cfg_name"])]
    w = iv.make_swin_weights(cfg, int(f["seed"]))
    sd = {str(k): torch.from_numpy(np.asarray(w[str(k)] if str(k) in w else f["buf/" + str(k)]).copy()) for k in f["keys"]}
    m = SwinTransformer(img_size=cfg.img_size, patch_size=cfg.patch_size, num_classes=cfg.num_classes,
                        embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads,
                        window_size=cfg.window_size, mlp_ratio=cfg.mlp_ratio)
    ck.load_reference_state_dict(m, {"state_dict": sd})
    imgs = iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"]))
    with torch.no_grad():
        acc, _ = m(dev(imgs))
    assert np.array_equal(acc.cpu().numpy(), g["logits_int"])
    scales = {n: np.float32(mod.act_scaling_factor.reshape(-1)[0].item()) for n, mod in m.named_modules()
              if type(mod) is iv.QuantAct and float(mod.act_scaling_factor.reshape(-1)[0]) > 0}
    eng = SwinEngine(cfg, w, scales)
    assert np.array_equal(eng.forward(dev(imgs)).cpu().numpy(), g["logits_int"])


def test_device_resize_center_crop_equals_oracle(H):
    """N3: ivit_resize_center_crop_u8 == the CPU restatement bit for bit (down- and up-scaling, portrait and landscape,
    batch > 1), and the whole eval transform (resize -> crop -> ToTensor -> Normalize -> input QuantAct) on the device
    equals the same chain built from the oracle's resize and torch's fp32 normalisation."""
    from oracle import oracle as orc
    from ivit_amd import preprocess as pp
    g = load_golden("resize.npz")
    for ci in range(int(g["n"])):
        size, crop = [int(v) for v in g[f"cfg/{ci}"]]
        img = np.concatenate([g[f"in/{ci}"], g[f"in/{ci}"][:, ::-1].copy()])       # batch of 2 (second one flipped)
        got = pp.resize_center_crop(dev(img), size, crop).cpu().numpy()
        assert np.array_equal(got, orc.resize_center_crop_u8(img, size, crop)), ci
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (3, 300, 400, 3), dtype=np.uint8)
    s_in = np.float32(0.0207)
    q = pp.eval_transform(dev(img), s_in, 256, 224).cpu().numpy()
    crop = orc.resize_center_crop_u8(img, 256, 224)
    x = torch.from_numpy(crop).permute(0, 3, 1, 2).float() / 255.0
    mean = torch.tensor(pp.IMAGENET_DEFAULT_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(pp.IMAGENET_DEFAULT_STD).view(1, 3, 1, 1)
    ref = torch.clamp(torch.round((1.0 / torch.tensor(s_in)) * ((x - mean) / std)), -128, 127).to(torch.int8).numpy()
    assert np.array_equal(q, ref)


@pytest.mark.parametrize("T,kind", [(197, "spread"), (197, "peaky"), (197, "saturated"), (577, "spread"), (577, "peaky"), (50, "saturated"),
                                    (1, "spread"), (64, "spread"), (65, "peaky"), (256, "spread"), (257, "saturated"), (640, "spread")])
def test_fused_attention_core_vs_oracle(H, T, kind):
    """the fused attention kernels against the CPU ORACLE directly (not against the unfused HIP chain):
    q.k^T -> qact_attn1 -> Shiftmax(16) -> attn.v -> qact2 (vit_quant.py:70-83) at the token counts of the 224- and
    384-pixel models and at the edges of the three kernel sizes (1, 64 | 65, 256 | 257, 640 keys: run-time token count, ragged
    last query tile, every wavefront-to-tile assignment), with score rows spread over the int8 range, peaky rows (one dominant
    key: the factor flips) and saturated rows (many scores clamped at +-127/-128); the arithmetic Shiftmax and both table-driven
    forms (two-level tables, row tables)."""
    from oracle import oracle as orc
    rng = np.random.default_rng(T + len(kind))
    B, Hh, dh = 2, 2, 64
    ld = (T + 15) // 16 * 16
    q = rng.integers(-128, 128, (B * Hh, T, dh), dtype=np.int8)
    k = rng.integers(-128, 128, (B * Hh, T, dh), dtype=np.int8)
    v = rng.integers(-128, 128, (B * Hh, T, dh), dtype=np.int8)
    scale = np.float32(0.1947)
    if kind == "peaky":
        k = (k.astype(np.int32) // 6).astype(np.int8)
        for r in range(T):                     # every query has one key it matches strongly
            k[:, (r * 7) % T, :] = q[:, r, :] // 2
        s_acc = np.float32(9.0e-5)
    elif kind == "saturated":
        s_acc = np.float32(2.4e-3)             # rq(acc) overshoots int8 on most of the row
    else:
        s_acc = np.float32(2.2e-4)
    dqk_h = iv.freeze.dyadic(s_acc, scale)
    dpv_h = iv.freeze.dyadic(np.float32(2.0 ** -15 * 0.1), np.float32(0.05))
    # ---- oracle: the four reference operators in sequence
    acc = orc.bmm_nt_i8(q, k)                                            # [BH, T, T]
    s8 = orc.requant(acc, orc.dyadic(s_acc, scale), 8).astype(np.int8)
    if kind == "saturated":
        assert (np.abs(s8.astype(np.int32)) >= 127).mean() > 0.3
    p16 = orc.shiftmax(s8, scale, 16)
    ctx = orc.bmm_av(p16, v)                                             # [BH, T, dh]
    ref = orc.requant(ctx, orc.dyadic(np.float32(2.0 ** -15 * 0.1), np.float32(0.05)), 8)
    ref = ref.reshape(B, Hh, T, dh).transpose(0, 2, 1, 3).reshape(B, T, Hh * dh)
    # ---- HIP
    vt = np.zeros((B * Hh, dh, ld), np.int8)
    vt[:, :, :T] = v.transpose(0, 2, 1)
    qd, kd, vd = dev(q), dev(k), dev(vt)
    o1 = torch.full((B, T, Hh * dh), 9, dtype=torch.int8, device="cuda")
    H.call("ivit_attention_fused", P(qd), P(kd), P(vd), dyv(dqk_h), float(scale), dyv(dpv_h), P(o1), B, Hh, T, dh, ld)
    assert np.array_equal(o1.cpu().numpy().astype(np.int32), ref), (T, kind, "arithmetic")
    tabs = iv.freeze.shiftmax_tables(scale)
    assert tabs is not None
    o2 = torch.full_like(o1, 9)
    H.call("ivit_attention_fused_lut", P(qd), P(kd), P(vd), dyv(dqk_h), float(scale), P(dev(tabs["aq"])), P(dev(tabs["t"])),
           P(dev(tabs["cls"])), int(tabs["NC"]), int(tabs["t"].size), int(tabs["dmin"]), dyv(dpv_h), P(o2), B, Hh, T, dh, ld)
    assert np.array_equal(o2.cpu().numpy().astype(np.int32), ref), (T, kind, "tables")
    rt = torch.empty(256, 64, dtype=torch.float32, device="cuda")
    H.call("ivit_shiftmax_rowtable", P(dev(tabs["aq"])), P(dev(tabs["t"])), P(dev(tabs["cls"])), int(tabs["NC"]), int(tabs["t"].size), int(tabs["dmin"]), P(rt))
    o3 = torch.full_like(o1, 9)
    H.call("ivit_attention_fused_rowlut", P(qd), P(kd), P(vd), dyv(dqk_h), float(scale), P(rt), int(tabs["dmin"]), dyv(dpv_h), P(o3), B, Hh, T, dh, ld)
    assert np.array_equal(o3.cpu().numpy().astype(np.int32), ref), (T, kind, "row tables")
    o4 = torch.full_like(o1, 9)              # the same with v ROW-major (ldv = 0): transposed inside the kernel
    H.call("ivit_attention_fused_rowlut", P(qd), P(kd), P(dev(v)), dyv(dqk_h), float(scale), P(rt), int(tabs["dmin"]), dyv(dpv_h), P(o4), B, Hh, T, dh, 0)
    assert np.array_equal(o4.cpu().numpy().astype(np.int32), ref), (T, kind, "row tables, v row-major")
    with pytest.raises(_lib.IvitError, match="ldv"):      # the other forms read v^T only
        H.call("ivit_attention_fused", P(qd), P(kd), P(vd), dyv(dqk_h), float(scale), dyv(dpv_h), P(o1), B, Hh, T, dh, 0)
    assert len(np.unique(ref)) > 10


@pytest.mark.parametrize("M", [640, 1000, 2 * 256 * 64 + 37, 3 * 256 * 64 + 64 * 5 + 1])
def test_mlp_fused_vs_oracle(H, M):
    """ivit_mlp_fused against the CPU ORACLE directly (Mlp.forward, layers_quant.py:144-153 + the residual
    QuantAct of the block): fc1 -> qact(8) -> ShiftGELU -> qact(8) -> fc2 -> qact(16) -> qact(16, + identity).
    640 / 1000 rows run the phase-by-phase kernel; from two 64-token tiles per CU on the role-split
    swin_mlp_rs_kernel runs: 32 805 rows (two tiles everywhere, a ragged third on one workgroup) and 49 473 (three, and a
    fourth on five workgroups plus a one-row tile)."""
    from oracle import oracle as orc
    rng = np.random.default_rng(M + 1)
    C, HD = 96, 384
    x = rng.integers(-128, 128, (M, C), dtype=np.int8)
    w1 = rng.integers(-128, 128, (HD, C), dtype=np.int8); b1 = rng.integers(-3000, 3000, HD).astype(np.int32)
    w2 = rng.integers(-128, 128, (C, HD), dtype=np.int8); b2 = rng.integers(-3000, 3000, C).astype(np.int32)
    s1 = (10 ** rng.uniform(-5.3, -4.9, HD)).astype(np.float32); s_h = np.float32(0.012)
    s_gelu_in = np.float32(0.03); s_g = np.float32(0.02)
    s2 = (10 ** rng.uniform(-5.6, -5.2, C)).astype(np.float32); s_t = np.float32(2e-4)
    s_res, s_fin = np.float32(2.7e-4), np.float32(3.1e-4)
    res = rng.integers(-30000, 30000, (M, C)).astype(np.int16)
    # oracle chain (the GELU input scale of the kernel's table is s_gelu_in: the hidden int8 IS the GELU input)
    h8 = orc.requant(orc.linear_i8(x, w1, b1), orc.dyadic(s1, s_h), 8).astype(np.int8)
    g16 = orc.shiftgelu(h8, s_gelu_in)
    g8 = orc.requant(g16.astype(np.int32), orc.dyadic(np.float32(s_gelu_in * np.float32(2.0 ** -7)), s_g), 8).astype(np.int8)
    t = orc.requant(orc.linear_i8(g8, w2, b2), orc.dyadic(s2, s_t), 16)
    ref = orc.requant(t, orc.dyadic(s_t, s_fin), 16, res.astype(np.int32), orc.dyadic(s_res, s_fin))
    tab = torch.empty(65536, dtype=torch.int8, device="cuda")
    H.call("ivit_shiftgelu_build_table", float(s_gelu_in), dyv(iv.freeze.dyadic(np.float32(s_gelu_in * np.float32(2.0 ** -7)), s_g)), P(tab))
    out = torch.full((M, C), -7, dtype=torch.int16, device="cuda")
    H.call("ivit_mlp_fused", P(dev(x)), P(dev(w1)), P(dev(b1)), P(dev(iv.freeze.dyadic(s1, s_h))), P(tab), P(dev(w2)), P(dev(b2)),
           P(dev(iv.freeze.dyadic(s2, s_t))), dyv(iv.freeze.dyadic(s_t, s_fin)), dyv(iv.freeze.dyadic(s_res, s_fin)), P(dev(res)), P(out), M, C, HD)
    assert np.array_equal(out.cpu().numpy().astype(np.int32), ref)


def test_swin_sliced_concurrency_stress():
    """Slices on internal streams must give the unsliced integers EVERY time: 8 slices x 25 forwards of Swin-T b256.  (Round 3:
    layernorm_reg_kernel<192, 1> returned one-LSB differences in a few rows when GEMM workgroups shared its CUs — 10-20 % of
    the sliced Swin forwards had a wrong image; the golden prefix of one image never showed it.  tools/swin_stress.py.)"""
    from ivit_amd.swin_engine import SwinEngine
    g = load_golden("swin_tiny_b1.npz")
    cfg = iv.SWIN_CONFIGS[str(g["cfg_name"])]
    eng = SwinEngine(cfg, iv.make_swin_weights(cfg, int(g["seed"])), golden_scales(g))
    B = 256
    imgs = np.concatenate([iv.make_images_int8(cfg, 1, int(g["images_seed"])), iv.make_images_int8(cfg, B - 1, seed=11)])
    d = dev(imgs)
    ref = eng.forward(d).clone().cpu().numpy()
    assert np.array_equal(ref[:1], g["logits_int"])
    for i in range(25):
        out = eng.forward(d, nslices=8).cpu().numpy()
        assert np.array_equal(out, ref), (i, np.nonzero((out != ref).any(1))[0])


def test_layernorm_beside_gemms_concurrency(H):
    """Every dispatched layernorm_reg_kernel shape launched on 8 streams at once, interleaved with QuantLinear GEMMs on the
    same streams: each output equals the single-stream result (tools/op_stress.py is the long form).  The K = 48 shape is the
    patch-embedding GEMM on gemm_nt_kernel (MFMA accumulators in AGPRs): the aggressor beside which the packed-fp32 form of the
    S = 1 LayerNorm failed in up to 40 % of its launches (profiles/r05_hazard/README.md)."""
    rng = np.random.default_rng(3)
    NS = 8
    streams = [torch.cuda.Stream() for _ in range(NS)]
    hs = [_lib.Handle(0, st.cuda_stream) for st in streams]
    ops = []
    for (K, N, M) in ((96, 288, 50176), (384, 1152, 6272), (48, 96, 100352)):
        x = dev(rng.integers(-128, 128, (M, K), dtype=np.int8)); w = dev(rng.integers(-128, 128, (N, K), dtype=np.int8))
        b = dev(rng.integers(-3000, 3000, N).astype(np.int32))
        d = dev(iv.freeze.dyadic((10 ** rng.uniform(-5.6, -5.2, N)).astype(np.float32), np.float32(0.012)))
        ops.append((lambda M=M, N=N: torch.empty(M, N, dtype=torch.int8, device="cuda"),
                    lambda h, o, x=x, w=w, b=b, d=d, M=M, N=N, K=K: h.call("ivit_linear_i8_requant", P(x), P(w), P(b), P(d), 8, P(o), M, N, K)))
    for (C, M) in ((96, 25088), (128, 12544), (192, 25088), (256, 6272), (384, 6272), (512, 3136), (768, 1568), (1024, 1568), (1536, 1568)):
        xx = dev(rng.integers(-20000, 20000, (M, C)).astype(np.int16))
        bb = dev(rng.normal(0, 3e5, C).astype(np.float32)); ss = dev((10 ** rng.uniform(-10.2, -9.8, C)).astype(np.float32))
        dd = dev(iv.freeze.dyadic((10 ** rng.uniform(-10.2, -9.8, C)).astype(np.float32), np.float32(0.03)))
        ops.append((lambda M=M, C=C: torch.empty(M, C, dtype=torch.int8, device="cuda"),
                    lambda h, o, xx=xx, bb=bb, ss=ss, dd=dd, M=M, C=C: h.call("ivit_layernorm_requant", P(xx), M, C, C, 0.01, P(bb), P(ss), P(dd), P(o))))
    refs = []
    for mk, call in ops:
        r = mk(); call(hs[0], r); torch.cuda.synchronize(); refs.append(r.clone())
    for rep in range(12):
        outs = [[mk() for mk, _ in ops] for _ in range(NS)]
        torch.cuda.synchronize()
        for j in range(len(ops)):
            for i in range(NS):
                k = (j + i * 3) % len(ops)
                ops[k][1](hs[i], outs[i][k])
        torch.cuda.synchronize()
        for i in range(NS):
            for k in range(len(ops)):
                assert torch.equal(outs[i][k], refs[k]), (rep, i, k)
    for h in hs:
        h.close()


# ---------------------------------------------------------------- the multi-rank paths on ONE GPU
def _run_ranks(args, env_extra, timeout):
    import os
    import socket
    import subprocess
    import sys
    from conftest import ROOT
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, IVIT_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), **env_extra)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port)] + args
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def test_bench_two_ranks_on_one_gpu():
    """bench.py's `world > 1` branch (broadcast of the constants blob, the barriers, the MAX all-reduce over ranks, the
    every-rank exit) had never executed on a GPU: run it as the driver launches it — torch.distributed.run, 2 ranks — with both
    ranks on device 0 and gloo as the transport (bench.py: IVIT_DIST_BACKEND, `local_rank % device_count`).  Then the same
    with a deliberately wrong golden: BOTH ranks must leave non-zero, promptly, and print no JSON line (the checks are --full's)."""
    import json
    import time
    args = ["bench.py", "--gpus", "2", "--model", "deit_tiny", "--batch", "8", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline",
            "--profile-steps", "0", "--min-seconds", "0", "--reps", "1"]
    r = _run_ranks(args, {}, 300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                      # ONE JSON line, from rank 0
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 16 and out["scaling"] == "weak"
    assert out["bit_exact_vs_reference_golden"] is True and out["all_images_equal_unsliced_forward"] is True
    assert out["value"] > 0 and abs(out["value"] - 16 * out["steps"] / (out["ms_per_step"] * 1e-3 * out["steps"])) < 1e-3 * out["value"]
    t0 = time.time()
    bad = _run_ranks(args, {"IVIT_BENCH_SELFTEST_WRONG_GOLDEN": "1"}, 300)
    assert bad.returncode != 0 and time.time() - t0 < 120
    assert not [ln for ln in bad.stdout.splitlines() if ln.startswith("{")], "a wrong golden prefix must not produce a bench line"
    assert "golden prefix differ" in bad.stderr


def test_bench_plain_run_dumps_last_step_logits(tmp_path):
    """a plain bench run (no --full) times exactly --steps steps once and prints the headline keys without the parts that take
    runs of their own; the logits it writes with --dump-outputs are the timed path's, for the seeded batch bench.py builds
    (golden images first, then seed 101): every image equals the CPU oracle's."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    from oracle import oracle as orc
    cmd = [sys.executable, "bench.py", "--model", "deit_tiny", "--batch", "8", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["unit"] == "images/s" and out["higher_is_better"] is True and out["dtype"] == "int8"
    assert out["steps"] == 3 and out["value_is"] == "one timed region of 3 steps"
    assert out["value"] > 0 and abs(out["value"] - 8 * 1e3 / out["ms_per_step"]) < 1e-3 * out["value"]
    assert not {"roofline", "box", "kernel_breakdown_ms", "cpu_baseline", "repetitions_ms_per_step"} & set(out)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["logits.npy"]
    got = np.load(tmp_path / "logits.npy")
    assert got.dtype == np.float64 and got.shape == (8, 1000)
    g = load_golden("deit_tiny_b1.npz")
    cfg = iv.CONFIGS["deit_tiny"]
    gb = int(g["batch"])
    imgs = np.concatenate([iv.make_images_int8(cfg, gb, int(g["images_seed"])), iv.make_images_int8(cfg, 8, seed=101)])[:8]
    ref, _ = orc.OracleViT(cfg, iv.make_vit_weights(cfg, int(g["seed"])), golden_scales(g)).forward(imgs)
    assert np.array_equal(ref[:gb], g["logits_int"])
    assert np.array_equal(got, ref.astype(np.float64))


def test_engine_forward_sharded_over_two_ranks():
    """SURVEY §4 multi-GPU row ("on 1 GPU simulate N shards") through the HIP ENGINE, not the oracle: two ranks receive the
    broadcast constants, each runs the native forward on its shard of 7 images (ragged: 4 + 3), the gathered logits equal
    the unsharded forward and the golden prefix (tools/dist_shard_check.py)."""
    r = _run_ranks(["tools/dist_shard_check.py", "micro_vit2h_b3.npz", "7"], {}, 300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "SHARD_CHECK_OK world 2 shards [(0, 4), (4, 7)]" in r.stdout
