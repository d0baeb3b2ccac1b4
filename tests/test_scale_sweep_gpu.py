"""The HIP library swept over activation scales and requant multipliers against the reference
(tests/golden/scale_sweep.npz, recorded from the reference's own modules by tools/make_scale_sweep_fixture.py; the CPU
oracle is pinned to the same fixture in tests/test_scale_sweep_cpu.py).  One test per operator; each loops over the
scales inside, reuses its buffers and reads the results back once.  Checksums are compared first; on a mismatch the
oracle at that scale names the operator, the scale and the number of differing elements.  Then the requant multiplier
bands of the attention kernels: the exact (non-fast) instantiation at and above 512, and window attention at its
refusal bounds."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from oracle import oracle as orc  # noqa: E402
import scale_sweep as sw  # noqa: E402
from test_swin_window12_gpu import chain_window_attention  # noqa: E402

_P = ctypes.c_void_p
f32 = np.float32


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def g():
    z = load_golden("scale_sweep.npz")
    return {k: z[k] for k in z.files}


_KEEP = []


def dev(a):
    """host -> device; the tensor is kept alive until the test ends (raw pointers are handed to the C-ABI, and a freed block
    is handed out again by the next allocation)"""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    _KEEP.append(t)
    return t


@pytest.fixture(autouse=True)
def _release_device_buffers():
    yield
    torch.cuda.synchronize()
    del _KEEP[:]


def P(t):
    return _P(t.data_ptr())


def dyv(d):
    """ivit_amd.freeze.dyadic array [n, 2] -> the by-value struct of its first entry"""
    return _lib.Dyadic(float(d[0, 0]), float(d[0, 1]))


def odv(d):
    """oracle.dyadic array -> the by-value struct of its first entry"""
    return _lib.Dyadic(float(d[0].m), float(d[0].r))


def status(H, name, *args):
    """the raw status code of an entry point (Handle.call raises on anything but IVIT_OK)"""
    return getattr(H.lib, name)(H.h, *args)


def check(got, want_csum, what, scale, ref):
    """checksum first; on a mismatch compare with the oracle at that scale"""
    if sw.csum(got) == want_csum:
        return
    r = np.asarray(ref()).astype(np.int64)
    n = int((np.asarray(got).astype(np.int64) != r).sum())
    raise AssertionError(f"{what} at scale {float(scale)!r}: checksum differs from the reference; {n} of {r.size} elements "
                         f"differ from the oracle (oracle checksum {'matches' if sw.csum(r) == want_csum else 'differs too'})")


# ---------------------------------------------------------------------------------------------- Shiftmax
def test_shiftmax_sweep(H, g):
    """ivit_shiftmax, 8 and 16 bit, ld_in / ld_out padded to 16 with poisoned pad columns that must stay untouched"""
    for n in sw.SHIFTMAX_N:
        x, bits = g[f"shiftmax/{n}/x"], sw.SHIFTMAX_BITS[n]
        scales, cs = g["ew/scales"], g[f"shiftmax/{n}/csum"]
        if bits == 16:
            scales, cs = np.concatenate([scales, g["attn/scales"]]), np.concatenate([cs, g[f"shiftmax/{n}/attn_csum"]])
        rows, ld = x.shape[0], (n + 15) // 16 * 16
        xp = np.full((rows, ld), 127, np.int8)              # a pad column read as a score would move the row maximum
        xp[:, :n] = x
        xd = dev(xp)
        out = torch.full((len(scales), rows, ld), 0x7777, dtype=torch.int16, device="cuda")
        for i, s in enumerate(scales):
            H.call("ivit_shiftmax", P(xd), rows, n, ld, float(s), bits, P(out[i]), ld)
        got = out.cpu().numpy().view(np.uint16)
        assert (got[:, :, n:] == 0x7777).all(), f"n={n}: pad columns written"
        for i, s in enumerate(scales):
            check(got[i, :, :n], cs[i], f"ivit_shiftmax n={n} bits={bits}", s, lambda: orc.shiftmax(x, s, bits))


def test_shiftmax_masked_sweep(H, g):
    """ivit_shiftmax_masked with the 0 / -100.0 mask of shifted windows (nW = 4, H = 3) and with mask == NULL"""
    x, mask = g["masked/x"], g["masked/mask"]
    rows, n = x.shape
    ld = 64
    xp = np.full((rows, ld), 127, np.int8)
    xp[:, :n] = x
    xd, md = dev(xp), dev(mask)
    scales = g["ew/scales"]
    out = torch.full((2, len(scales), rows, ld), 0x7777, dtype=torch.int16, device="cuda")
    for i, s in enumerate(scales):
        H.call("ivit_shiftmax_masked", P(xd), rows, n, ld, float(s), 8, P(md), sw.MASK_NW, sw.MASK_H, P(out[0, i]), ld)
        H.call("ivit_shiftmax_masked", P(xd), 259, n, ld, float(s), 8, None, sw.MASK_NW, sw.MASK_H, P(out[1, i]), ld)
    got = out.cpu().numpy().view(np.uint16)
    assert (got[:, :, :, n:] == 0x7777).all() and (got[1, :, 259:] == 0x7777).all()
    for i, s in enumerate(scales):
        check(got[0, i, :, :n], g["masked/csum"][i], "ivit_shiftmax_masked", s,
              lambda: orc.shiftmax_masked(x, s, 8, mask, sw.MASK_NW, sw.MASK_H))
        check(got[1, i, :259, :n], g["shiftmax/49/csum"][i], "ivit_shiftmax_masked(mask=NULL)", s,
              lambda: orc.shiftmax(x[:259], s, 8))


# ---------------------------------------------------------------------------------------------- ShiftGELU
def test_shiftgelu_sweep(H, g):
    """The four ShiftGELU entry points on the block of every (row max, Q) pair.  The 16-bit form refuses exactly the scales
    at which the fixture's recorded extremes of Q*sigmoid_int leave int16 (IVIT_ERR_UNSUPPORTED, the message names the scale,
    nothing is written) and equals the reference at every other scale; the 8-bit forms carry the product in 32 bits and
    equal the reference at every scale, the overflowing ones included."""
    x = g["gelu/x"]
    xd = dev(x)
    scales = g["ew/scales"]
    S = len(scales)
    over = (g["gelu/min"] < -32768) | (g["gelu/max"] > 32767)
    assert over.any() and not over.all()
    o16 = torch.full((S, 256, 256), 0x5555, dtype=torch.int16, device="cuda")
    o8 = torch.full((S, 2, 3, 256, 256), 0x55, dtype=torch.int8, device="cuda")      # direct | table | table form
    for i, s in enumerate(scales):
        st = status(H, "ivit_shiftgelu", P(xd), 256, 256, float(s), P(o16[i]))
        if over[i]:
            assert st == _lib.IVIT_ERR_UNSUPPORTED, f"scale {float(s)!r}: |Q*sig| reaches {int(g['gelu/maxabs'][i])}, status {st}"
            assert f"{float(s):.9g}" in H.lib.ivit_last_error(H.h).decode()
        else:
            assert st == _lib.IVIT_OK, f"scale {float(s)!r} fits int16 (|Q*sig| <= {int(g['gelu/maxabs'][i])}) and was refused"
        for j in range(2):
            dy = dyv(iv.freeze.dyadic(f32(s * f32(2.0 ** -7)), g["gelu/s_out8"][i, j]))
            H.call("ivit_shiftgelu_requant", P(xd), 256, 256, float(s), dy, P(o8[i, j, 0]))
            H.call("ivit_shiftgelu_build_table", float(s), dy, P(o8[i, j, 1]))
            H.call("ivit_shiftgelu_requant_lut", P(xd), 256, 256, P(o8[i, j, 1]), P(o8[i, j, 2]))
    o16, o8 = o16.cpu().numpy(), o8.cpu().numpy()
    tri = np.tril(np.ones((256, 256), bool))                  # table entries with Q <= row max: the block itself
    for i, s in enumerate(scales):
        if over[i]:
            assert (o16[i] == 0x5555).all(), f"refused call wrote its output at scale {float(s)!r}"
        else:
            check(o16[i], g["gelu/csum"][i], "ivit_shiftgelu", s, lambda: orc.shiftgelu32(x, s))
        for j in range(2):
            def ref():
                return orc.requant(orc.shiftgelu32(x, s), orc.dyadic(f32(s * f32(2.0 ** -7)), g["gelu/s_out8"][i, j]), 8)
            check(o8[i, j, 0], g["gelu/csum8"][i, j], "ivit_shiftgelu_requant", s, ref)
            check(o8[i, j, 2], g["gelu/csum8"][i, j], "ivit_shiftgelu_build_table + ivit_shiftgelu_requant_lut", s, ref)
            # the table on its indexed half is the direct form's output on this block
            assert np.array_equal(o8[i, j, 1][tri], o8[i, j, 0][tri]), f"ivit_shiftgelu_build_table at scale {float(s)!r}"


# ---------------------------------------------------------------------------------------------- I-LayerNorm
def test_layernorm_sweep(H, g):
    s_out = g["ln/s_out"]
    scales = g["ln/scales"]
    for C in sw.LN_C:
        x = g[f"ln/{C}/x"]
        rows = x.shape[0]
        bias_int, sc = iv.freeze.layernorm_constants(g[f"ln/{C}/w"], g[f"ln/{C}/b"])
        xd, bd, sd, dd = dev(x), dev(bias_int), dev(sc), dev(iv.freeze.dyadic(sc, s_out))
        z = torch.full((len(scales), rows, C), float("nan"), dtype=torch.float32, device="cuda")
        o8 = torch.full((len(scales), rows, C), 0x55, dtype=torch.int8, device="cuda")
        for i, s in enumerate(scales):
            H.call("ivit_layernorm", P(xd), rows, C, float(s), P(bd), P(sd), P(z[i]))
            H.call("ivit_layernorm_requant", P(xd), rows, C, C, float(s), P(bd), P(sd), P(dd), P(o8[i]))
        z, o8 = z.cpu().numpy(), o8.cpu().numpy()
        assert np.isfinite(z).all()
        for i, s in enumerate(scales):
            check(z[i].astype(np.float64), g[f"ln/{C}/csum_z"][i], f"ivit_layernorm C={C}", s,
                  lambda: orc.layernorm(x, s, bias_int, sc))
            check(o8[i], g[f"ln/{C}/csum8"][i], f"ivit_layernorm_requant C={C}", s,
                  lambda: orc.requant(orc.layernorm(x, s, bias_int, sc), orc.dyadic(sc, s_out), 8))


def test_layernorm_tokenorder_sweep(H, g):
    """The token-order kernels (Swin stage 0) on two images of 49 tokens: C = 96 and 128 run layernorm_tokenorder8_kernel,
    C = 64 and 192 the run-time-C kernel.  z and the 8-bit result against the reference's IntLayerNorm on a token-contiguous
    input; ivit_patch_norm_tokenorder (int8 input, two 16-bit QuantActs) against the chain of oracle.layernorm_ord, which the
    CPU file pins to the same fixture."""
    s_out, L = g["ln/s_out"], sw.LN_TOKENS
    scales = g["ln/scales"]
    s_a, s_b = f32(3.1e-4), f32(4.7e-4)
    for C in sw.LN_TOKEN_C:
        x, w, b = sw.ln_token_block(C)
        rows = x.shape[0]
        x8 = (x >> 8).astype(np.int8)
        bias_int, sc = iv.freeze.layernorm_constants(w, b)
        xd, x8d, bd, sd = dev(x), dev(x8), dev(bias_int), dev(sc)
        d8, d16 = dev(iv.freeze.dyadic(sc, s_out)), dev(iv.freeze.dyadic(sc, s_a))
        dy2 = dyv(iv.freeze.dyadic(s_a, s_b))
        z = torch.full((len(scales), rows, C), float("nan"), dtype=torch.float32, device="cuda")
        o8 = torch.full((len(scales), rows, C), 0x55, dtype=torch.int8, device="cuda")
        o16 = torch.full((len(scales), rows, C), 0x5555, dtype=torch.int16, device="cuda")
        for i, s in enumerate(scales):
            H.call("ivit_layernorm_tokenorder", P(xd), rows, C, float(s), P(bd), P(sd), L, P(z[i]))
            H.call("ivit_layernorm_tokenorder_requant", P(xd), rows, C, float(s), P(bd), P(sd), P(d8), L, P(o8[i]))
            H.call("ivit_patch_norm_tokenorder", P(x8d), rows, C, float(s), P(bd), P(sd), P(d16), dy2, L, P(o16[i]))
        z, o8, o16 = z.cpu().numpy(), o8.cpu().numpy(), o16.cpu().numpy()
        for i, s in enumerate(scales):
            check(z[i].astype(np.float64), g[f"lntok/{C}/csum_z"][i], f"ivit_layernorm_tokenorder C={C}", s,
                  lambda: orc.layernorm_ord(x, s, bias_int, sc, 1, L))
            check(o8[i], g[f"lntok/{C}/csum8"][i], f"ivit_layernorm_tokenorder_requant C={C}", s,
                  lambda: orc.requant(orc.layernorm_ord(x, s, bias_int, sc, 1, L), orc.dyadic(sc, s_out), 8))
            a = orc.requant(orc.layernorm_ord(x8.astype(np.int16), s, bias_int, sc, 1, L), orc.dyadic(sc, s_a), 16)
            ref = orc.requant(a, orc.dyadic(s_a, s_b), 16)
            assert np.array_equal(o16[i], ref), \
                f"ivit_patch_norm_tokenorder C={C} at scale {float(s)!r}: {int((o16[i] != ref).sum())} of {ref.size} elements differ"


# ---------------------------------------------------------------------------------------------- QuantAct
def test_quantize_input_sweep(H, g):
    scales = g["qin/scales"]
    n = g["qin/grid"].size
    ld = (n + 15) // 16 * 16                              # every scale's block starts 16-byte aligned; n itself is odd
    xh = np.zeros((len(scales), ld), f32)
    xh[:, :n] = np.stack([sw.qin_values(s) for s in scales])
    xs = dev(xh)
    q = torch.full((len(scales), ld), 0x55, dtype=torch.int8, device="cuda")
    for i, s in enumerate(scales):
        H.call("ivit_quantize_input_f32", P(xs[i]), float(s), P(q[i]), n)
    q = q.cpu().numpy()
    assert (q[:, n:] == 0x55).all(), "elements past n written"
    for i, s in enumerate(scales):
        check(q[i, :n], g["qin/csum"][i], "ivit_quantize_input_f32", s, lambda: orc.quantize_f32(sw.qin_values(s), s, 8))


def test_requant_multiplier_sweep(H, g):
    """ivit_requant_i32 / _i16 / _f32 over per-channel multipliers from 2^-30 to 2^12 and beyond (both float32 neighbours of
    512, 1024, 2048 and 2^31 / max|z|), exact .5 ties, 8 and 16 bits, with and without an identity branch: the reference's
    own outputs"""
    zid = dev(g["rq/z_id"])
    for ci, (zname, bits, ident) in enumerate(sw.RQ_CASES):
        z, ratios = g[f"rq/{zname}/z"], g[f"rq/{zname}/ratios"]
        want = g[f"rq/out/{ci}"]
        dy = dev(iv.freeze.dyadic((ratios * sw.RQ_S_OUT).astype(f32), sw.RQ_S_OUT))
        dyi = dev(iv.freeze.dyadic(f32(sw.RQ_ID_RATIO[ident] * sw.RQ_S_OUT), sw.RQ_S_OUT)) if ident else None
        forms = [("ivit_requant_i32", z), ("ivit_requant_f32", z.astype(f32))]
        if zname == "z16":
            forms.append(("ivit_requant_i16", z.astype(np.int16)))
        for name, zz in forms:
            out = torch.full(z.shape, 0x55, dtype=torch.int8 if bits == 8 else torch.int16, device="cuda")
            H.call(name, P(dev(zz)), P(dy), sw.RQ_C, P(zid) if ident else None, P(dyi) if ident else None, bits, P(out),
                   z.shape[0], sw.RQ_C)
            got = out.cpu().numpy()
            bad = np.unique(np.nonzero(got != want)[1])
            assert bad.size == 0, f"{name} case {ci} ({zname}, {bits} bit, identity {ident}): {int((got != want).sum())} elements " \
                                  f"differ, at multipliers {ratios[bad].tolist()}"


# ---------------------------------------------------------------------------------------------- attention
def _attention_ref(q, k, v, dqk, s, dpv, B, Hh):
    """the four reference operators in sequence (vit_quant.py:70-83), as in test_fused_attention_core_vs_oracle; the Shiftmax
    in it is pinned to the reference at these scales by the fixture"""
    T, dh = q.shape[1], q.shape[2]
    s8 = orc.requant(orc.bmm_nt_i8(q, k), dqk, 8).astype(np.int8)
    ctx = orc.bmm_av(orc.shiftmax(s8, s, 16), v)
    ref = orc.requant(ctx, dpv, 8)
    return ref.reshape(B, Hh, T, dh).transpose(0, 2, 1, 3).reshape(B, T, Hh * dh).astype(np.int8), s8


def _vt(v, ld):
    BH, T, dh = v.shape
    vt = np.zeros((BH, dh, ld), np.int8)
    vt[:, :, :T] = v.transpose(0, 2, 1)
    return vt


def _run_attention_forms(H, q, k, v, dqk, s, dpv, B, Hh, tabs, rowtab_ok=True):
    """-> {form: int8 output}: every attention entry point that applies at this scale; whole-T forms [B, T, H*dh], class-token
    forms [B, H*dh]"""
    T, dh = q.shape[1], q.shape[2]
    ld = (T + 15) // 16 * 16
    qd, kd, vd, vr = dev(q), dev(k), dev(_vt(v, ld)), dev(v)
    outs = {}

    def new(cls):
        return torch.full((B, Hh * dh) if cls else (B, T, Hh * dh), 0x55, dtype=torch.int8, device="cuda")

    outs["fused"] = o = new(False)
    H.call("ivit_attention_fused", P(qd), P(kd), P(vd), dqk, float(s), dpv, P(o), B, Hh, T, dh, ld)
    outs["fused_cls"] = o = new(True)
    H.call("ivit_attention_fused_cls", P(qd), P(kd), P(vd), dqk, float(s), dpv, P(o), None, None, B, Hh, T, dh, ld)
    if tabs is not None:
        aq, et, cl = dev(tabs["aq"]), dev(tabs["t"]), dev(tabs["cls"])
        targs = (P(aq), P(et), P(cl), int(tabs["NC"]), int(tabs["t"].size), int(tabs["dmin"]))
        outs["lut"] = o = new(False)
        H.call("ivit_attention_fused_lut", P(qd), P(kd), P(vd), dqk, float(s), *targs, dpv, P(o), B, Hh, T, dh, ld)
        outs["lut_cls"] = o = new(True)
        H.call("ivit_attention_fused_lut_cls", P(qd), P(kd), P(vd), dqk, float(s), *targs, dpv, P(o), None, None, B, Hh, T, dh, ld)
        if rowtab_ok and tabs["R"] <= 64:
            rt = torch.full((256, 64), float("nan"), dtype=torch.float32, device="cuda")
            H.call("ivit_shiftmax_rowtable", *targs, P(rt))
            dmin = int(tabs["dmin"])
            outs["rowtab"] = rt
            outs["rowlut"] = o = new(False)
            H.call("ivit_attention_fused_rowlut", P(qd), P(kd), P(vd), dqk, float(s), P(rt), dmin, dpv, P(o), B, Hh, T, dh, ld)
            outs["rowlut_vrow"] = o = new(False)
            H.call("ivit_attention_fused_rowlut", P(qd), P(kd), P(vr), dqk, float(s), P(rt), dmin, dpv, P(o), B, Hh, T, dh, 0)
            outs["rowlut_cls"] = o = new(True)
            H.call("ivit_attention_fused_rowlut_cls", P(qd), P(kd), P(vd), dqk, float(s), P(rt), dmin, dpv, P(o), None, None, B, Hh, T, dh, ld)
    return {n: o.cpu().numpy() for n, o in outs.items()}


def _compare_forms(outs, ref, what):
    for name, got in outs.items():
        if name == "rowtab":
            continue
        want = ref[:, 0, :] if name.endswith("_cls") else ref
        assert np.array_equal(got, want), f"{what}, form {name}: {int((got != want).sum())} of {want.size} elements differ from the oracle chain"


def _spread_qkv(rng, BH, T, dh=64):
    """q rows of growing amplitude, so that the maxima of the score rows differ"""
    q = rng.integers(-128, 128, (BH, T, dh)).astype(np.int32)
    q = (q * ((np.arange(T) % 8 + 1) / 8.0)[None, :, None]).astype(np.int8)
    k = rng.integers(-128, 128, (BH, T, dh), dtype=np.int8)
    v = rng.integers(-128, 128, (BH, T, dh), dtype=np.int8)
    return q, k, v


def test_attention_sweep(H, g):
    """Every fused attention form — arithmetic, two-level tables, row tables with v^T and with row-major v, and the three
    class-token forms — at every attention scale: T = 17 (one key block) and T = 65 (four key blocks), T = 257 (ten) at five of
    the scales.  A scale without tables runs the arithmetic form only; a scale whose row-table line needs more than 64
    entries gets IVIT_ERR_UNSUPPORTED from ivit_shiftmax_rowtable; the device-built row table equals
    freeze.shiftmax_rowtable."""
    scales = g["attn/scales"]
    B, Hh = 1, 2
    big = set(np.linspace(0, len(scales) - 4, 5).round().astype(int).tolist())
    dpv_s = (f32(2.0 ** -15 * 0.1), f32(0.05))
    seen = {"none": 0, "tables": 0, "rowtable": 0, "refused": 0}
    for i, s in enumerate(scales):
        tabs = iv.freeze.shiftmax_tables(s)
        host_rt = iv.freeze.shiftmax_rowtable(tabs)
        seen["none" if tabs is None else "rowtable" if host_rt is not None else "tables"] += 1
        if tabs is not None and tabs["R"] > 64:
            rt = torch.full((256, 64), 7.0, dtype=torch.float32, device="cuda")
            st = status(H, "ivit_shiftmax_rowtable", P(dev(tabs["aq"])), P(dev(tabs["t"])), P(dev(tabs["cls"])), int(tabs["NC"]),
                        int(tabs["t"].size), int(tabs["dmin"]), P(rt))
            assert st == _lib.IVIT_ERR_UNSUPPORTED and (rt.cpu().numpy() == 7.0).all(), (float(s), tabs["R"], st)
            seen["refused"] += 1
        for T in (17, 65) + ((257,) if i in big else ()):
            rng = np.random.default_rng(1000 * i + T)
            q, k, v = _spread_qkv(rng, B * Hh, T)
            s_acc = f32(1.14e-3 * s)                        # acc has a deviation near 4.4e4 * the row's amplitude: scores spread over int8
            ref, s8 = _attention_ref(q, k, v, orc.dyadic(s_acc, s), s, orc.dyadic(*dpv_s), B, Hh)
            assert len(np.unique(s8.max(axis=-1))) >= 8 and len(np.unique(ref)) > 10
            outs = _run_attention_forms(H, q, k, v, dyv(iv.freeze.dyadic(s_acc, s)), s, dyv(iv.freeze.dyadic(*dpv_s)), B, Hh, tabs)
            _compare_forms(outs, ref, f"attention at scale {float(s)!r}, T={T}")
            if "rowtab" in outs:
                assert np.array_equal(outs["rowtab"], host_rt), f"ivit_shiftmax_rowtable at scale {float(s)!r}"
    assert seen["none"] >= 1 and seen["refused"] >= 1 and seen["rowtable"] * 3 >= len(scales), seen


def test_window_attention_sweep(H, g):
    """ivit_window_attention_fused and _lut (window 7) at twelve of the attention scales, with and without the shift mask,
    against the oracle chain of tests/test_swin_window12_gpu.py"""
    scales = g["attn/scales"]
    pick = np.argsort(scales, kind="stable")[np.linspace(0, len(scales) - 1, 12).round().astype(int)]
    B, R, heads = 1, 14, 3
    lut_runs = 0
    for i in pick:
        s = scales[i]
        tabs = iv.freeze.shiftmax_tables(s)
        for shift in (0, 3):
            rng = np.random.default_rng(50 * int(i) + shift)
            qkv = rng.integers(-128, 128, (B, R, R, 3, heads, 32), dtype=np.int8)
            relb = rng.integers(-40, 41, (heads, 49, 49)).astype(np.int16)
            s_attn1 = f32(1.3 * s)
            dqk = orc.dyadic(f32(s_attn1 * 2.4e-3), s_attn1)    # acc has a deviation near 3.1e4: scores spread over int8
            da = orc.dyadic(s_attn1, s)
            dpv = orc.dyadic(f32(2.0 ** -7 * 0.031), f32(0.029))
            ref = chain_window_attention(qkv, relb, dqk, da, dpv, s, R, shift, heads, ws=7)
            assert len(np.unique(ref)) > 10
            dq, dr = dev(qkv), dev(relb)
            out = torch.full((B, R * R, heads * 32), 0x55, dtype=torch.int8, device="cuda")
            H.call("ivit_window_attention_fused", P(dq), odv(dqk), odv(da), P(dr), float(s), odv(dpv), P(out), B, R, 7, shift, heads, 32)
            got = out.cpu().numpy()
            assert np.array_equal(got, ref), f"ivit_window_attention_fused at scale {float(s)!r}, shift {shift}: {int((got != ref).sum())} differ"
            if tabs is not None:
                out = torch.full_like(out, 0x55)
                H.call("ivit_window_attention_fused_lut", P(dq), odv(dqk), odv(da), P(dr), float(s), P(dev(tabs["aq"])), P(dev(tabs["t"])),
                       P(dev(tabs["cls"])), int(tabs["NC"]), int(tabs["t"].size), int(tabs["dmin"]), odv(dpv), P(out), B, R, 7, shift, heads, 32)
                got = out.cpu().numpy()
                assert np.array_equal(got, ref), f"ivit_window_attention_fused_lut at scale {float(s)!r}, shift {shift}: {int((got != ref).sum())} differ"
                lut_runs += 1
    assert lut_runs >= 8


# ---------------------------------------------------------------------------------------------- the multiplier bands
def _mult(v):
    """a dyadic whose multiplier m * 2^-e is exactly the float32 value v (a 24-bit mantissa fits m's 31 bits)"""
    d = orc.dyadic(f32(f32(v) * f32(2.0 ** -6)), f32(2.0 ** -6))
    assert d[0].m * d[0].r == float(f32(v))
    return d


def _sparse_qk(rng, BH, T, dh):
    """q.k^T in {-1, 0, 1}: a multiplier of 512 or more turns any other accumulator into a saturated score.  A third of the
    query rows are zero (flat score rows), the others hold one +-1."""
    q = np.zeros((BH, T, dh), np.int8)
    k = np.zeros((BH, T, dh), np.int8)
    for b in range(BH):
        for t in range(T):
            if t % 3:
                q[b, t, rng.integers(0, dh)] = rng.choice([-1, 1])
            k[b, t, rng.integers(0, dh, 3 * dh // 8)] = rng.choice([-1, 1], 3 * dh // 8)
    return q, k


def _half_zero_v(rng, shape):
    """v with every other channel zero: under a multiplier of 512 or more those channels stay 0, the others saturate"""
    v = rng.integers(-128, 128, shape, dtype=np.int8)
    v[..., ::2] = 0
    return v


BELOW_512, ABOVE_512 = np.nextafter(f32(512), f32(0)), np.nextafter(f32(512), f32(1024))


@pytest.mark.parametrize("T", [17, 65])
def test_attention_exact_instantiation_bands(H, T):
    """attn_fused_kernel<NB, false, ...> serves requant multipliers at or above 512.  ivit_attention_fused and _lut (with their
    class-token forms) against the oracle chain with dy_qk multipliers just below 512, exactly 512 and 600, and dy_pv
    multipliers just below and just above 512; the data saturate part of the scores / outputs, not all.  The row-table form
    refuses the out-of-range cases."""
    B, Hh, dh = 1, 2, 64
    s = f32(0.1947)
    tabs = iv.freeze.shiftmax_tables(s)
    assert tabs is not None and tabs["R"] <= 64
    rng = np.random.default_rng(T)
    small_pv = orc.dyadic(f32(2.0 ** -15 * 0.1), f32(0.05))
    cases = []
    for m in (BELOW_512, f32(512), f32(600)):
        q, k = _sparse_qk(rng, B * Hh, T, dh)
        cases.append((f"dy_qk {float(m)!r}", q, k, rng.integers(-128, 128, (B * Hh, T, dh), dtype=np.int8), _mult(m), small_pv))
    for m in (BELOW_512, ABOVE_512):
        q, k, _ = _spread_qkv(rng, B * Hh, T)
        cases.append((f"dy_pv {float(m)!r}", q, k, _half_zero_v(rng, (B * Hh, T, dh)), orc.dyadic(f32(1.14e-3 * s), s), _mult(m)))
    for what, q, k, v, dqk, dpv in cases:
        ref, s8 = _attention_ref(q, k, v, dqk, s, dpv, B, Hh)
        sat_s = (np.abs(s8.astype(np.int32)) >= 127).mean()
        sat_o = ((ref == 127) | (ref == -128)).mean()
        share = sat_s if what.startswith("dy_qk") else sat_o
        assert 0.1 < share < 0.9, (what, share)                          # part of the rows, not all
        fast = abs(dqk[0].m * dqk[0].r) < 512 and abs(dpv[0].m * dpv[0].r) < 512
        outs = _run_attention_forms(H, q, k, v, odv(dqk), s, odv(dpv), B, Hh, tabs, rowtab_ok=fast)
        assert ("rowlut" in outs) == fast
        _compare_forms(outs, ref, f"attention T={T}, {what}")
        if not fast:
            ld = (T + 15) // 16 * 16
            rt = dev(iv.freeze.shiftmax_rowtable(tabs))
            o = torch.full((B, T, Hh * dh), 0x55, dtype=torch.int8, device="cuda")
            st = status(H, "ivit_attention_fused_rowlut", P(dev(q)), P(dev(k)), P(dev(_vt(v, ld))), odv(dqk), float(s), P(rt),
                        int(tabs["dmin"]), odv(dpv), P(o), B, Hh, T, dh, ld)
            assert st == _lib.IVIT_ERR_UNSUPPORTED and (o.cpu().numpy() == 0x55).all(), (what, st)


@pytest.mark.parametrize("window,R,heads", [(7, 14, 3), (12, 12, 2)])
def test_window_attention_at_its_refusal_bounds(H, window, R, heads):
    """Window attention refuses dy_qk multipliers from 2048 and dy_pv multipliers from 1024 (IVIT_ERR_INVALID, the poisoned
    output untouched); just below either bound (2047.9, 1023.9) it equals the oracle chain."""
    B, N = 1, window * window
    s = f32(0.1947)
    shift = window // 2 if R > window else 0
    rng = np.random.default_rng(window)
    relb = rng.integers(-40, 41, (heads, N, N)).astype(np.int16)
    da = orc.dyadic(f32(0.21), s)
    normal_qk, normal_pv = orc.dyadic(f32(0.21 * 2.4e-3), f32(0.21)), orc.dyadic(f32(2.0 ** -7 * 0.031), f32(0.029))
    # sparse q | k (accumulators in {-1, 0, 1}) with a random v for the dy_qk band; random q | k with a half-zero v for the dy_pv band
    qkv_qk = np.zeros((B, R, R, 3, heads, 32), np.int8)
    q, k = _sparse_qk(rng, B * R * R, heads, 32)
    qkv_qk[:, :, :, 0], qkv_qk[:, :, :, 1] = q.reshape(B, R, R, heads, 32), k.reshape(B, R, R, heads, 32)
    qkv_qk[:, :, :, 2] = rng.integers(-128, 128, (B, R, R, heads, 32))
    qkv_pv = rng.integers(-128, 128, (B, R, R, 3, heads, 32), dtype=np.int8)
    qkv_pv[:, :, :, 2] = _half_zero_v(rng, (B, R, R, heads, 32))
    tabs = iv.freeze.shiftmax_tables(s)
    dr = dev(relb)

    def run(qkv, dqk, dpv, lut):
        out = torch.full((B, R * R, heads * 32), 0x55, dtype=torch.int8, device="cuda")
        if lut:
            st = status(H, "ivit_window_attention_fused_lut", P(dev(qkv)), odv(dqk), odv(da), P(dr), float(s), P(dev(tabs["aq"])),
                        P(dev(tabs["t"])), P(dev(tabs["cls"])), int(tabs["NC"]), int(tabs["t"].size), int(tabs["dmin"]), odv(dpv),
                        P(out), B, R, window, shift, heads, 32)
        else:
            st = status(H, "ivit_window_attention_fused", P(dev(qkv)), odv(dqk), odv(da), P(dr), float(s), odv(dpv), P(out), B, R,
                        window, shift, heads, 32)
        return st, out.cpu().numpy()

    for what, qkv, dqk, dpv, ok in (("dy_qk 2047.9", qkv_qk, _mult(2047.9), normal_pv, True), ("dy_qk 2048", qkv_qk, _mult(2048), normal_pv, False),
                                    ("dy_pv 1023.9", qkv_pv, normal_qk, _mult(1023.9), True), ("dy_pv 1024", qkv_pv, normal_qk, _mult(1024), False)):
        for lut in (False, True) if window == 7 else (False,):
            st, got = run(qkv, dqk, dpv, lut)
            if not ok:
                assert st == _lib.IVIT_ERR_INVALID and (got == 0x55).all(), (what, lut, st)
                continue
            assert st == _lib.IVIT_OK, (what, lut, st, H.lib.ivit_last_error(H.h).decode())
            ref = chain_window_attention(qkv, relb, dqk, da, dpv, s, R, shift, heads, ws=window)
            sat = ((ref == 127) | (ref == -128)).mean()
            assert (0.02 < sat < 0.98) if what.startswith("dy_pv") else len(np.unique(ref)) > 10, (what, sat)
            assert np.array_equal(got, ref), f"window {window}, {what}, lut={lut}: {int((got != ref).sum())} of {ref.size} elements differ"
