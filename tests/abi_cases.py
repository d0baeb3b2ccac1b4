"""The C-ABI's call table, shared by tests/test_twin.py (HIP library == CPU twin) and the memory-contract tests
(tests/test_memory_contract_cpu.py, tests/test_memory_contract_gpu.py).

`_cases(rng, variant)`: one valid argument list per TWINNED entry point.  `hip_cases(H, rng)`: the entries that have no twin or need
a plan protocol.  An argument is a scalar / Dyadic, None, ("host", array), ("ref", key) — a handle the case's setup closure made —
or ("in" | "out", array[, pad]).  `pad` describes bytes inside the array that are not payload:
    an int n           columns >= n of the last axis: an input's pad columns, an output's columns the entry does not write;
    ("zero", n)        an input's pad columns that include/ivit.h REQUIRES to be zero;
    ("free", mask)     an output of which only mask's bytes are pinned (the others may or may not be written).
`ALIGN` records, per entry and activation argument, what happens when that one pointer is element-aligned but not 16-byte aligned.
`INPLACE` records the (input, output) pairs an entry accepts at the same address; every other overlap of an output with an activation
input or another output is refused (`check_overlap`).  `twin_table`, `hip_table` and `cases_of` are the tables as the contract tests
read them, built once per seed; `check_stream_contract` runs one case on a side stream inside a hipGraph capture and replays it
(tests/test_stream_graph_contract_gpu.py).

The second half is the arena harness: every array in its own [guard | payload | guard] allocation, on numpy or on the device."""
import ctypes
import functools
import os
import sys

import numpy as np

from conftest import ROOT

import ivit_amd as iv
from ivit_amd import _lib

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_twin_header  # noqa: E402

_P = ctypes.c_void_p

def hp(a):
    return a.ctypes.data_as(_P)


def dyv(d):
    return _lib.Dyadic(float(d[0, 0]), float(d[0, 1]))


def load_twin():
    """the CPU twin (oracle/libivit_oracle.so, built on demand) with the C-ABI's own ctypes signatures"""
    from oracle import oracle as orc
    return _lib.bind(ctypes.CDLL(orc.build()), gen_twin_header.TWIN, prefix="ivit_cpu_")     # AttributeError = a declared twin is not exported


def _io():
    """the two argument tags: I(array[, pad]) / O(array[, pad])"""
    return (lambda a, *pad: ("in", np.ascontiguousarray(a)) + pad), (lambda a, *pad: ("out", a) + pad)


# ---------------------------------------------------------------- the same calls through both libraries
def _cases(rng, variant=0):
    """-> list of (entry point, args); an argument is a scalar / Dyadic, ("in", array), ("out", array) or None.
    variant 1 is a second argument list per entry point: ragged row counts, other channel / token counts, other scales."""
    I, O = _io()
    cs = []
    V = variant
    M, N, K = ((300, 96, 64), (173, 160, 128))[V]
    x = rng.integers(-128, 128, (M, K), dtype=np.int8)
    w = np.rint(rng.normal(0, 40, (N, K)).clip(-127, 127)).astype(np.int8)
    b = rng.integers(-3000, 3000, N).astype(np.int32)
    s_pre = (10 ** rng.uniform(*((-5.5, -4.5), (-5.1, -4.2))[V], N)).astype(np.float32)
    d8, d16 = iv.freeze.dyadic(s_pre, np.float32((2e-2, 3.1e-2)[V])), iv.freeze.dyadic(s_pre, np.float32((1e-4, 1.7e-4)[V]))
    dm, dr = iv.freeze.dyadic(np.float32(1e-4), np.float32(2e-4)), iv.freeze.dyadic(np.float32(3e-4), np.float32(2e-4))
    res = rng.integers(-20000, 20000, (M, N)).astype(np.int16)
    cs.append(("quantize_input_f32", [I(rng.normal(0, 1, 5000).astype(np.float32)), 0.02, O(np.zeros(5000, np.int8)), 5000]))
    cs.append(("linear_i8", [I(x), I(w), I(b), O(np.zeros((M, N), np.int32)), M, N, K]))
    cs.append(("linear_i8_requant", [I(x), I(w), I(b), I(d8), 8, O(np.zeros((M, N), np.int8)), M, N, K]))
    cs.append(("linear_i8_requant", [I(x), I(w), I(b), I(d16), 16, O(np.zeros((M, N), np.int16)), M, N, K]))
    cs.append(("linear_i8_requant_residual", [I(x), I(w), I(b), I(d16), dyv(dm), dyv(dr), I(res), O(np.zeros((M, N), np.int16)), M, N, K]))
    # attention-shaped entry points: B = 2, H = 2, T = 50, dh = 64
    B, Hh, T, dh, ld = ((2, 2, 50, 64, 64), (3, 1, 37, 64, 48))[V]
    D = Hh * dh
    xq = rng.integers(-128, 128, (B * T, D), dtype=np.int8)
    wq = np.rint(rng.normal(0, 30, (3 * D, D)).clip(-127, 127)).astype(np.int8)
    bq = rng.integers(-3000, 3000, 3 * D).astype(np.int32)
    dq = iv.freeze.dyadic((10 ** rng.uniform(-5.5, -5.0, 3 * D)).astype(np.float32), np.float32(4e-2))
    q = rng.integers(-128, 128, (B * Hh, T, dh), dtype=np.int8)
    k = rng.integers(-128, 128, (B * Hh, T, dh), dtype=np.int8)
    vt = np.zeros((B * Hh, dh, ld), np.int8)
    vt[:, :, :T] = rng.integers(-128, 128, (B * Hh, dh, T), dtype=np.int8)
    dqk, dpv = iv.freeze.dyadic(np.float32(2e-4), np.float32(6e-2)), iv.freeze.dyadic(np.float32(3e-6), np.float32(9e-3))
    cs.append(("linear_i8_qkv", [I(xq), I(wq), I(bq), I(dq), O(np.zeros((B * Hh, T, dh), np.int8)), O(np.zeros((B * Hh, T, dh), np.int8)),
                                 O(np.zeros((B * Hh, dh, ld), np.int8), T), B, T, Hh, dh, ld]))
    cs.append(("bmm_nt_i8", [I(q), I(k), O(np.zeros((B * Hh, T, T), np.int32)), B * Hh, T, T, dh, dh, dh, T, T * dh, T * dh, T * T]))
    p16 = np.zeros((B * Hh, T, ld), np.uint16)
    p16[:, :, :T] = rng.integers(0, 32769, (B * Hh, T, T)).astype(np.uint16)
    cs.append(("bmm_nt_u16i8", [I(p16, T), I(vt, T), O(np.zeros((B * Hh, T, dh), np.int32)), B * Hh, T, dh, T, ld, ld, dh, T * ld, dh * ld, T * dh]))
    cs.append(("attn_qk_requant", [I(q), I(k), dyv(dqk), O(np.zeros((B * Hh, T, ld), np.int8), T), B * Hh, T, dh, ld]))
    cs.append(("attn_pv_requant", [I(p16, T), I(vt, T), dyv(dpv), O(np.zeros((B, T, D), np.int8)), B, Hh, T, dh, ld, ld]))
    cs.append(("attention_fused", [I(q), I(k), I(vt, T), dyv(dqk), 0.06, dyv(dpv), O(np.zeros((B, T, D), np.int8)), B, Hh, T, dh, ld]))
    # requant flavours
    z32 = rng.integers(-2 ** 20, 2 ** 20, (M, N)).astype(np.int32)
    zid = rng.integers(-30000, 30000, (M, N)).astype(np.int32)
    cs.append(("requant_i32", [I(z32), I(d8), N, None, None, 8, O(np.zeros((M, N), np.int8)), M, N]))
    cs.append(("requant_i32", [I(z32), I(dm), 1, I(zid), I(dr), 16, O(np.zeros((M, N), np.int16)), M, N]))
    cs.append(("requant_i16", [I(res), I(dm), 1, None, None, 16, O(np.zeros((M, N), np.int16)), M, N]))
    cs.append(("requant_f32", [I(z32.astype(np.float32) * 4096.0), I(iv.freeze.dyadic(s_pre * np.float32(1e-3), np.float32(2e-2))), N,
                               None, None, 8, O(np.zeros((M, N), np.int8)), M, N]))
    # elementwise operators
    R8 = (64, 61)[V]
    s8 = rng.integers(-128, 128, (R8, 197), dtype=np.int8)
    s8[3] = -128; s8[4] = 127; s8[5, :] = -100; s8[5, 17] = 90                       # flat, saturated and peaky rows
    cs.append(("shiftmax", [I(s8), R8, 197, 197, (0.07, 0.093)[V], 16, O(np.zeros((R8, 197), np.uint16)), 197]))
    cs.append(("shiftmax", [I(s8), R8, 197, 197, (0.11, 0.157)[V], 8, O(np.zeros((R8, 197), np.uint16)), 197]))
    Rg, Cg, sg = ((40, 384, 0.03), (37, 768, 0.045))[V]
    g8 = rng.integers(-128, 128, (Rg, Cg), dtype=np.int8)
    g8[2] = rng.integers(-128, -60, Cg, dtype=np.int8)                                # an all-negative row
    dg = iv.freeze.dyadic(np.float32(sg * 2.0 ** -7), np.float32((0.025, 0.033)[V]))
    tab = np.zeros(65536, np.int8)
    cs.append(("shiftgelu", [I(g8), Rg, Cg, sg, O(np.zeros((Rg, Cg), np.int16))]))
    cs.append(("shiftgelu_requant", [I(g8), Rg, Cg, sg, dyv(dg), O(np.zeros((Rg, Cg), np.int8))]))
    idx = np.arange(65536)                  # entries with Q > row max are never indexed (the twin leaves them 0)
    cs.append(("shiftgelu_build_table", [sg, dyv(dg), O(tab, ("free", (idx & 255) <= (idx >> 8)))]))
    C = (192, 384)[V]
    Rl = (48, 50)[V]
    xl = rng.integers(-9000, 9000, (Rl, C)).astype(np.int16)
    xl[1] = 1234                                                                       # a zero-variance row
    wl, bl = rng.uniform(0.4, 1.6, C).astype(np.float32), rng.normal(0, 0.3, C).astype(np.float32)
    wl[5] = -0.7
    bias_int, sc = iv.freeze.layernorm_constants(wl, bl)
    dl = iv.freeze.dyadic(sc, np.float32(0.03))
    sl = (2.5e-4, 3.3e-4)[V]
    cs.append(("layernorm", [I(xl), Rl, C, sl, I(bias_int), I(sc), O(np.zeros((Rl, C), np.float32))]))
    cs.append(("layernorm_requant", [I(xl), Rl, C, C, sl, I(bias_int), I(sc), I(dl), O(np.zeros((Rl, C), np.int8))]))
    # one channel with a multiplier far above the |z * c| < 2^31 bound: the block takes the v_rndne_f64 / saturating form of the
    # 8-bit requant (ivit_layernorm.h) instead of the magic-number one
    dl_wide = dl.copy()
    dl_wide[3:4] = iv.freeze.dyadic(sc[3:4], np.float32(1e-13))
    cs.append(("layernorm_requant", [I(xl), Rl, C, C, sl, I(bias_int), I(sc), I(dl_wide), O(np.zeros((Rl, C), np.int8))]))
    img = rng.integers(-128, 128, (2, 3, 32, 32), dtype=np.int8)
    cs.append(("im2col_patch", [I(img), 2, 3, 32, 32, 8, O(np.zeros((2 * 16, 3 * 64), np.int8))]))
    Te, De = ((17, 64), (10, 128))[V]
    cs.append(("embed_finish", [I(rng.integers(-20000, 20000, (2, Te - 1, De)).astype(np.int16)), I(rng.integers(-10 ** 6, 10 ** 6, De).astype(np.int32)),
                                I(rng.integers(-20000, 20000, (Te, De)).astype(np.int16)), dyv(dm), dyv(dr), O(np.zeros((2, Te, De), np.int16)), 2, Te, De]))
    # ---- round 3: Swin-specific operators
    a49 = rng.integers(-128, 128, (8 * 3 * 49, 49), dtype=np.int8)                     # [B_ = 8, H = 3, 49] rows
    mk = np.where(rng.random((4, 49, 49)) < 0.3, np.float32(-100.0), np.float32(0.0)).astype(np.float32)
    cs.append(("shiftmax_masked", [I(a49), 8 * 3 * 49, 49, 49, 0.05, 8, I(mk), 4, 3, O(np.zeros((8 * 3 * 49, 49), np.uint16)), 49]))
    cs.append(("shiftmax_masked", [I(a49), 8 * 3 * 49, 49, 49, 0.05, 8, None, 0, 0, O(np.zeros((8 * 3 * 49, 49), np.uint16)), 49]))
    zb = rng.integers(-128, 128, 6 * 3 * 2401).astype(np.int32)
    zi = rng.integers(-128, 128, 3 * 2401).astype(np.int32)
    da, db = iv.freeze.dyadic(np.float32(0.04), np.float32(0.05)), iv.freeze.dyadic(np.float32(0.01), np.float32(0.05))
    cs.append(("requant_i32_bcast", [I(zb), dyv(da), I(zi), 3 * 2401, dyv(db), 8, O(np.zeros(6 * 3 * 2401, np.int8)), 6 * 3 * 2401]))
    cs.append(("avgpool_requant", [I(rng.integers(-128, 128, (3, 49, 96), dtype=np.int8)), 3, 49, 96, dyv(iv.freeze.dyadic(np.float32(0.03), np.float32(0.02))),
                                   O(np.zeros((3, 96), np.int8))]))
    Ct, Lt = ((96, 64), (128, 49))[V]                                                   # token-order sums: 2 images of Lt tokens
    xt = rng.integers(-9000, 9000, (2 * Lt, Ct)).astype(np.int16)
    wt, bt = rng.uniform(0.4, 1.6, Ct).astype(np.float32), rng.normal(0, 0.3, Ct).astype(np.float32)
    bit, sct = iv.freeze.layernorm_constants(wt, bt)
    dt8, dt16 = iv.freeze.dyadic(sct, np.float32(0.03)), iv.freeze.dyadic(sct, np.float32(2e-4))
    cs.append(("layernorm_tokenorder", [I(xt), 2 * Lt, Ct, 2.5e-4, I(bit), I(sct), Lt, O(np.zeros((2 * Lt, Ct), np.float32))]))
    cs.append(("layernorm_tokenorder_requant", [I(xt), 2 * Lt, Ct, 2.5e-4, I(bit), I(sct), I(dt8), Lt, O(np.zeros((2 * Lt, Ct), np.int8))]))
    cs.append(("patch_norm_tokenorder", [I(rng.integers(-128, 128, (2 * Lt, Ct), dtype=np.int8)), 2 * Lt, Ct, 0.02, I(bit), I(sct), I(dt16),
                                         dyv(iv.freeze.dyadic(np.float32(2e-4), np.float32(2.5e-4))), Lt, O(np.zeros((2 * Lt, Ct), np.int16))]))
    pm = rng.integers(-20000, 20000, (2, 14, 14, 96)).astype(np.int16)
    cs.append(("patch_merge_gather", [I(pm), 16, 2, 14, 96, O(np.zeros((2, 49, 384), np.int16))]))
    cs.append(("patch_merge_gather", [I(rng.integers(-128, 128, (2, 14, 14, 96), dtype=np.int8)), 8, 2, 14, 96, O(np.zeros((2, 49, 384), np.int16))]))
    cs.append(("widen_i8_i16", [I(rng.integers(-128, 128, 5000, dtype=np.int8)), O(np.zeros(5000, np.int16)), 5000]))
    # windowed attention: 2 images of 14 x 14 tokens (2 x 2 windows), 3 heads, with and without the cyclic shift
    Bw, Rw, Hw = ((2, 14, 3), (1, 21, 2))[V]
    qkvw = rng.integers(-128, 128, (Bw, Rw, Rw, 3 * Hw * 32), dtype=np.int8)
    relb = rng.integers(-60, 60, (Hw, 49, 49)).astype(np.int16)
    dwq, dwa, dwp = (iv.freeze.dyadic(np.float32(a), np.float32(b)) for a, b in (((3e-4, 0.05), (0.05, 0.06), (4e-4, 0.03)), ((2.2e-4, 0.043), (0.043, 0.071), (5e-4, 0.026)))[V])
    for sh in (0, 3):
        cs.append(("window_attention_fused", [I(qkvw), dyv(dwq), dyv(dwa), I(relb), (0.06, 0.071)[V], dyv(dwp), O(np.zeros((Bw, Rw * Rw, Hw * 32), np.int8)),
                                              Bw, Rw, 7, sh, Hw, 32]))
    wtab = iv.freeze.shiftmax_tables(np.float32((0.06, 0.071)[V]))
    for sh in (0, 3):
        cs.append(("window_attention_fused_lut", [I(qkvw), dyv(dwq), dyv(dwa), I(relb), (0.06, 0.071)[V], I(wtab["aq"]), I(wtab["t"]), I(wtab["cls"]),
                                                  int(wtab["NC"]), int(wtab["t"].size), int(wtab["dmin"]), dyv(dwp),
                                                  O(np.zeros((Bw, Rw * Rw, Hw * 32), np.int8)), Bw, Rw, 7, sh, Hw, 32]))
    # ---- the uint8 front end (N3): ToTensor -> Normalize -> input QuantAct; antialiased bicubic resize + centre crop
    u8 = rng.integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)
    u8.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    mean, std = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
    cs.append(("normalize_quantize_u8", [I(u8), 2, 37, 53, ("host", mean), ("host", std), 0.0207, O(np.zeros((2, 3, 37, 53), np.int8))]))
    big = rng.integers(0, 256, (2, 60, 83, 3), dtype=np.uint8)
    cs.append(("resize_center_crop_u8", [I(big), 2, 60, 83, 40, 32, O(np.zeros((2, 60, 32, 3), np.float32)), O(np.zeros((2, 32, 32, 3), np.uint8))]))
    tall = rng.integers(0, 256, (1, 75, 50, 3), dtype=np.uint8)                        # portrait, upscaling
    cs.append(("resize_center_crop_u8", [I(tall), 1, 75, 50, 64, 56, O(np.zeros((1, 75, 56, 3), np.float32)), O(np.zeros((1, 56, 56, 3), np.uint8))]))
    return cs


def _marshal(handle, args, to_ptr, refs=None):
    """-> (the C argument list of the call, what to_ptr returned beside the pointer for every ("out", ...) argument)"""
    outs, call = [], [handle]
    for a in args:
        if isinstance(a, tuple) and a[0] == "host":          # a HOST array on both sides (mean / std of the normalisation)
            call.append(a[1].ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        elif isinstance(a, tuple) and a[0] == "ref":         # a plan handle or a device constant the case's setup made
            call.append(refs[a[1]])
        elif isinstance(a, tuple):
            buf = to_ptr(a[1], a[0] == "out")
            call.append(buf[0])
            if a[0] == "out":
                outs.append(buf[1])
        else:
            call.append(a)
    return call, outs


def _run(fn, handle, args, to_ptr, refs=None, status=0):
    call, outs = _marshal(handle, args, to_ptr, refs)
    st = fn(*call)
    assert st == status, st
    return outs


# ---------------------------------------------------------------- entries without a twin, or behind a plan protocol
def _layer(rng, N, K, bits):
    """a frozen QuantLinear K -> N with a `bits`-bit QuantAct behind it: (w, bias, per-channel dyadics)"""
    w = np.rint(rng.normal(0, 40, (N, K)).clip(-127, 127)).astype(np.int8)
    b = rng.integers(-3000, 3000, N).astype(np.int32)
    s_pre = (10 ** rng.uniform(-5.5, -5.0, N) * np.sqrt(384.0 / K)).astype(np.float32)
    return w, b, iv.freeze.dyadic(s_pre, np.float32({8: 3e-2, 16: 1.5e-4}[bits]))


def _ln(rng, C, s_out=0.031):
    """LayerNorm constants with gammas of both signs: (bias_int, sc, per-channel dyadics of the 8-bit QuantAct behind it)"""
    wln = rng.normal(1.0, 0.4, C).astype(np.float32) * rng.choice([-1.0, 1.0], C).astype(np.float32)
    bias_int, sc = iv.freeze.layernorm_constants(wln, rng.normal(0.0, 0.5, C).astype(np.float32))
    return bias_int, sc, iv.freeze.dyadic(sc, np.float32(s_out))


def _x16(rng, M, C):
    x = rng.integers(-20000, 20000, (M, C)).astype(np.int16)
    x[:, : C // 2] //= 64
    if M >= 3:
        x[1] = 1234                                       # a zero-variance row
    return x


LN_LDS_SCALE = 7.3e-4


@functools.lru_cache(maxsize=None)
def ln_lds_case(C):
    """Eight rows of C channels (row 3 constant: zero variance), the LayerNorm constants and the oracle's fp32 result at the input
    scale LN_LDS_SCALE; computed once per C and left unchanged.  ivit_layernorm asks for 8 * C * 4 bytes of dynamic LDS: above 64 KB
    from C = 2056 on (tests/test_gpu_parity.py, tests/test_stream_graph_contract_gpu.py)."""
    from oracle import oracle as orc
    rng = np.random.default_rng(C)
    w = rng.normal(1.0, 0.4, C).astype(np.float32) * rng.choice([-1.0, 1.0], C).astype(np.float32)
    bias_int, sc = iv.freeze.layernorm_constants(w, rng.normal(0.0, 0.5, C).astype(np.float32))
    x = rng.integers(-26000, 26000, (8, C)).astype(np.int16)
    x[:, : C // 2] //= 64                                         # small and large magnitudes in one row
    x[3] = 1234
    return x, bias_int, sc, orc.layernorm(x, LN_LDS_SCALE, bias_int, sc)


S_GELU, S_G_OUT = np.float32(0.03), np.float32(0.02)
ATT_SCALE = np.float32(0.1947)                            # a Shiftmax scale whose row-table lines fit 64 entries


def _setup(H, layers=(), prepare=(), mlp=None, select=0, cu_share=0, gelu=False, const=()):
    """-> setup closure of a case: device copies of the frozen layers, ivit_linear_plan_create (+ _prepare_ws for the keys in
    `prepare`), ivit_mlp_plan_create over the two keys of `mlp` (+ ivit_mlp_plan_select), the ShiftGELU table, further constants
    (name, array) on plain 256-byte-aligned allocations, the handle's CU share.  Calling it returns (refs, teardown)."""
    def setup():
        import torch
        keep, refs, plans, mp = [], {}, [], None
        up = lambda a: keep.append(torch.from_numpy(np.ascontiguousarray(a)).cuda()) or _P(keep[-1].data_ptr())
        for key, (w, b, d) in layers:
            p = _P()
            H.call("ivit_linear_plan_create", up(w), up(b), up(d), w.shape[0], w.shape[1], ctypes.byref(p))
            plans.append(p)
            refs[key] = p
            if key in prepare:
                H.call("ivit_linear_plan_prepare_ws", p)
        if mlp:
            mp = _P()
            H.call("ivit_mlp_plan_create", refs[mlp[0]], refs[mlp[1]], ctypes.byref(mp))
            assert H.lib.ivit_mlp_plan_select(mp, select) == 0
            refs["mlp"] = mp
        if gelu:
            keep.append(torch.empty(65536, dtype=torch.int8, device="cuda"))
            refs["tab"] = _P(keep[-1].data_ptr())
            H.call("ivit_shiftgelu_build_table", float(S_GELU), dyv(iv.freeze.dyadic(np.float32(S_GELU * 2.0 ** -7), S_G_OUT)), refs["tab"])
        for name, a in const:
            refs[name] = up(a)
        H.set_cu_share(cu_share)

        def teardown():
            torch.cuda.synchronize()
            H.set_cu_share(0)
            if mp is not None:
                assert H.lib.ivit_mlp_plan_destroy(mp) == 0
            for p in plans:
                assert H.lib.ivit_linear_plan_destroy(p) == 0
            del keep[:]
        return refs, teardown

    def host_refs(twin):
        """the same handles for the CPU twin (host pointers), or None for a case behind a plan: -> (refs, keep-alive)"""
        assert not layers
        keep, refs = [], {}
        if gelu:
            keep.append(np.zeros(65536, np.int8))         # the twin leaves the entries no row can index at 0; nobody reads them
            assert twin.ivit_cpu_shiftgelu_build_table(None, float(S_GELU), dyv(iv.freeze.dyadic(np.float32(S_GELU * 2.0 ** -7), S_G_OUT)),
                                                       hp(keep[-1])) == 0
            refs["tab"] = hp(keep[-1])
        for name, a in const:
            keep.append(np.ascontiguousarray(a))
            refs[name] = hp(keep[-1])
        return refs, keep
    setup.host_refs, setup.plans = host_refs, bool(layers)
    return setup


def _device_cus(H):
    """CUs of the handle's device, as ivit_create reads them (hipDeviceProp_t::multiProcessorCount); 256, an MI355X, without a handle"""
    if H is None:
        return 256
    import torch
    return torch.cuda.get_device_properties(H.device).multi_processor_count


def hip_cases(H, rng):
    """-> list of (entry point, args, setup): the entries that have no twin or need a plan protocol, at the smallest shapes that
    leave a partial tile in every tiled dimension of the kernel that serves the call ("one tile plus one row"), and on both sides of
    every size at which a launcher changes kernels.  setup is None or a closure -> (refs, teardown); ("ref", key) arguments are
    looked up in refs.  H may be None where only the names are wanted (the closures are not called)."""
    I, O = _io()
    R = lambda key: ("ref", key)
    cs = []
    add = lambda name, args, setup=None: cs.append((name, args, setup))
    i8 = lambda *shape: rng.integers(-128, 128, shape, dtype=np.int8)
    i16 = lambda *shape: rng.integers(-20000, 20000, shape).astype(np.int16)
    dm, dr = iv.freeze.dyadic(np.float32(2e-4), np.float32(3.1e-4)), iv.freeze.dyadic(np.float32(2.7e-4), np.float32(3.1e-4))

    # ---- planned QuantLinear layers.  A plan as created: gemm_ps_kernel (128-row tiles) from M = 128, gemm_as_kernel (256-row
    # units, K = 384) from M = 256, the launch-per-tile gemm_glds_kernel below; a prepared plan: gemm_ws_qkv_kernel (32-token tiles)
    l8, l16, lres = _layer(rng, 384, 384, 8), _layer(rng, 384, 384, 16), _layer(rng, 768, 384, 16)
    l192, l192r = _layer(rng, 576, 192, 8), _layer(rng, 192, 192, 16)
    for M in (17, 129, 257):
        add("linear_i8_requant_planned", [R("p"), I(i8(M, 384)), 8, O(np.zeros((M, 384), np.int8)), M], _setup(H, [("p", l8)]))
        add("linear_i8_requant_planned", [R("p"), I(i8(M, 384)), 16, O(np.zeros((M, 384), np.int16)), M], _setup(H, [("p", l16)]))
        add("linear_i8_requant_residual_planned", [R("p"), I(i8(M, 384)), dyv(dm), dyv(dr), I(i16(M, 768)), O(np.zeros((M, 768), np.int16)), M],
            _setup(H, [("p", lres)]))
    for lay, K in ((l8, 384), (l192, 192)):
        N, M = lay[0].shape[0], 33
        bi, sc, dln = _ln(rng, K)
        add("linear_i8_requant_planned", [R("p"), I(i8(M, K)), 8, O(np.zeros((M, N), np.int8)), M], _setup(H, [("p", lay)], prepare=("p",)))
        add("layernorm_linear_i8_requant_planned", [R("p"), I(_x16(rng, M, K)), 2.5e-4, R("bi"), R("sc"), R("dln"), O(np.zeros((M, N), np.int8)), M],
            _setup(H, [("p", lay)], prepare=("p",), const=(("bi", bi), ("sc", sc), ("dln", dln))))
    for lay, K in ((l16, 384), (l192r, 192)):
        M = 33
        add("linear_i8_requant_residual_planned", [R("p"), I(i8(M, K)), dyv(dm), dyv(dr), I(i16(M, K)), O(np.zeros((M, K), np.int16)), M],
            _setup(H, [("p", lay)], prepare=("p",)))
    bi, sc, dln = _ln(rng, 384)
    add("linear_i8_requant_residual_layernorm_planned",
        [R("p"), I(i8(33, 384)), dyv(dm), dyv(dr), I(i16(33, 384)), O(np.zeros((33, 384), np.int16)), 33, 3.1e-4, R("bi"), R("sc"), R("dln"),
         O(np.zeros((33, 384), np.int8))], _setup(H, [("p", l16)], prepare=("p",), const=(("bi", bi), ("sc", sc), ("dln", dln))))
    # the qkv scatter: D = 384 (six heads) on a plan as created (B*T = 130: gemm_ps_kernel, 260: gemm_as_kernel, 34: gemm_glds_kernel)
    # with v^T, on a prepared plan with v row-major; D = 192 prepared in both layouts of v; norm1 in the same launch
    lq384, lq192 = _layer(rng, 1152, 384, 8), l192
    for B, T in ((2, 17), (2, 65), (4, 65)):
        ld = (T + 15) // 16 * 16
        add("linear_i8_qkv_planned", [R("p"), I(i8(B * T, 384)), O(np.zeros((B * 6, T, 64), np.int8)), O(np.zeros((B * 6, T, 64), np.int8)),
                                      O(np.zeros((B * 6, 64, ld), np.int8), T), B, T, 6, 64, ld], _setup(H, [("p", lq384)]))
    for lay, K, Hh in ((lq384, 384, 6), (lq192, 192, 3)):
        bi, sc, dln = _ln(rng, K)
        ln = dict(prepare=("p",), const=(("bi", bi), ("sc", sc), ("dln", dln)))
        for B, T in ((2, 17), (1, 65)):
            ld = (T + 15) // 16 * 16
            qk = lambda: O(np.zeros((B * Hh, T, 64), np.int8))
            add("linear_i8_qkv_planned", [R("p"), I(i8(B * T, K)), qk(), qk(), qk(), B, T, Hh, 64, 0], _setup(H, [("p", lay)], prepare=("p",)))
            add("layernorm_linear_i8_qkv_planned", [R("p"), I(_x16(rng, B * T, K)), 2.5e-4, R("bi"), R("sc"), R("dln"), qk(), qk(), qk(), B, T, Hh, 64],
                _setup(H, [("p", lay)], **ln))
            add("layernorm_linear_i8_qkv_ldv_planned", [R("p"), I(_x16(rng, B * T, K)), 2.5e-4, R("bi"), R("sc"), R("dln"), qk(), qk(), qk(), B, T, Hh, 64, 0],
                _setup(H, [("p", lay)], **ln))
            if K == 192:
                vt = lambda: O(np.zeros((B * Hh, 64, ld), np.int8), T)
                add("linear_i8_qkv_planned", [R("p"), I(i8(B * T, K)), qk(), qk(), vt(), B, T, Hh, 64, ld], _setup(H, [("p", lay)], prepare=("p",)))
                add("layernorm_linear_i8_qkv_ldv_planned", [R("p"), I(_x16(rng, B * T, K)), 2.5e-4, R("bi"), R("sc"), R("dln"), qk(), qk(), vt(), B, T, Hh, 64, ld],
                    _setup(H, [("p", lay)], **ln))
    # ---- unplanned layers: the 8-bit QuantAct stored as int16 (gemm_glds_kernel at its 128-row tile: launch_gemm2 gives the 128-row
    # tile four resident slots per CU against two of the 256-row tile, so its cost estimate never picks the 256-row instantiation, at
    # any M, N or CU count — tests/test_memory_contract_cpu.py::test_glds_256_row_tile_is_unreachable), and the weights-in-registers
    # streaming kernel (gemm_wreg_kernel) that ivit_linear_i8_requant / _residual take from M = 8192 on at K = 96 / 128 / 192
    for M, N, K in ((129, 96, 64), (300, 160, 128)):
        w, b, d = _layer(rng, N, K, 8)
        add("linear_i8_requant8_store16", [I(i8(M, K)), I(w), I(b), I(d), O(np.zeros((M, N), np.int16)), M, N, K])
    for M, N, K in ((8209, 96, 96), (8209, 192, 192)):
        w, b, d = _layer(rng, N, K, 8)
        add("linear_i8_requant", [I(i8(M, K)), I(w), I(b), I(d), 8, O(np.zeros((M, N), np.int8)), M, N, K])
        w, b, d = _layer(rng, N, K, 16)
        add("linear_i8_requant", [I(i8(M, K)), I(w), I(b), I(d), 16, O(np.zeros((M, N), np.int16)), M, N, K])
        add("linear_i8_requant_residual", [I(i8(M, K)), I(w), I(b), I(d), dyv(dm), dyv(dr), I(i16(M, N)), O(np.zeros((M, N), np.int16)), M, N, K])
    # the kernel behind the in-place pair of INPLACE that no other case reaches: K = 48 is below gemm_glds_kernel's shapes
    # (gemm_nt_kernel, 128-row tiles: two whole ones and a ragged third)
    w, b, d = _layer(rng, 96, 48, 16)
    add("linear_i8_requant_residual", [I(i8(257, 48)), I(w), I(b), I(d), dyv(dm), dyv(dr), I(i16(257, 96)), O(np.zeros((257, 96), np.int16)), 257, 96, 48])

    # ---- whole-T fused attention in its table forms, and the class-token forms: T = 17 (one ragged 16-row query tile + 1) and 65
    tabs = iv.freeze.shiftmax_tables(ATT_SCALE)
    rowtab = iv.freeze.shiftmax_rowtable(tabs)
    assert rowtab is not None
    tconst = (("aq", tabs["aq"]), ("et", tabs["t"]), ("cl", tabs["cls"]), ("rt", rowtab))
    targs = [R("aq"), R("et"), R("cl"), int(tabs["NC"]), int(tabs["t"].size), int(tabs["dmin"])]
    dqk = iv.freeze.dyadic(np.float32(2.2e-4), ATT_SCALE)
    dpv = iv.freeze.dyadic(np.float32(2.0 ** -15 * 0.1), np.float32(0.05))
    add("shiftmax_rowtable", [I(tabs["aq"]), I(tabs["t"]), I(tabs["cls"]), int(tabs["NC"]), int(tabs["t"].size), int(tabs["dmin"]),
                              O(np.zeros((256, 64), np.float32))])
    B, Hh, dh = 2, 2, 64
    D = Hh * dh
    for T in (17, 65):
        ld = (T + 15) // 16 * 16
        q, k, v = i8(B * Hh, T, dh), i8(B * Hh, T, dh), i8(B * Hh, T, dh)
        vt = np.zeros((B * Hh, dh, ld), np.int8)
        vt[:, :, :T] = v.transpose(0, 2, 1)
        x16 = rng.integers(-32768, 32768, (B * T, D)).astype(np.int16)
        st = _setup(H, const=tconst)
        ctx, cls, xc = (lambda: O(np.zeros((B, T, D), np.int8))), (lambda: O(np.zeros((B, D), np.int8))), (lambda: O(np.zeros((B, D), np.int16)))
        shape = [B, Hh, T, dh]
        add("attention_fused_lut", [I(q), I(k), I(vt, T), dyv(dqk), float(ATT_SCALE)] + targs + [dyv(dpv), ctx()] + shape + [ld], st)
        add("attention_fused_rowlut", [I(q), I(k), I(vt, T), dyv(dqk), float(ATT_SCALE), R("rt"), int(tabs["dmin"]), dyv(dpv), ctx()] + shape + [ld], st)
        add("attention_fused_rowlut", [I(q), I(k), I(v), dyv(dqk), float(ATT_SCALE), R("rt"), int(tabs["dmin"]), dyv(dpv), ctx()] + shape + [0], st)
        add("attention_fused_cls", [I(q), I(k), I(vt, T), dyv(dqk), float(ATT_SCALE), dyv(dpv), cls(), I(x16), xc()] + shape + [ld])
        add("attention_fused_cls", [I(q), I(k), I(vt, T), dyv(dqk), float(ATT_SCALE), dyv(dpv), cls(), None, None] + shape + [ld])
        add("attention_fused_lut_cls", [I(q), I(k), I(vt, T), dyv(dqk), float(ATT_SCALE)] + targs + [dyv(dpv), cls(), I(x16), xc()] + shape + [ld], st)
        add("attention_fused_rowlut_cls", [I(q), I(k), I(vt, T), dyv(dqk), float(ATT_SCALE), R("rt"), int(tabs["dmin"]), dyv(dpv), cls(), I(x16), xc()] + shape + [ld], st)
        add("attention_fused_rowlut_cls", [I(q), I(k), I(v), dyv(dqk), float(ATT_SCALE), R("rt"), int(tabs["dmin"]), dyv(dpv), cls(), I(x16), xc()] + shape + [0], st)
    add("gather_rows_i16", [I(i16(3 * 17, 64)), 3, 64, 17 * 64, O(np.zeros((3, 64), np.int16))])

    # ---- ShiftGELU by table, and the fused Mlp kernels
    add("shiftgelu_requant_lut", [I(i8(37, 384)), 37, 384, R("tab"), O(np.zeros((37, 384), np.int8))], _setup(H, gelu=True))
    # C = 96: 64-row tiles, and from two tiles per CU of the DEVICE on (ivit_mlp_fused sizes by the device's CU count, not the handle's
    # share) the role-split kernel: the third M is the smallest count on that side plus a ragged tile
    for C, Ms in ((96, (17, 65, 2 * _device_cus(H) * 64 + 17)), (128, (17, 81))):
        HD = 4 * C
        (w1, b1, d1), (w2, b2, d2) = _layer(rng, HD, C, 8), _layer(rng, C, HD, 16)
        for M in Ms:
            add("mlp_fused", [I(i8(M, C)), I(w1), I(b1), I(d1), R("tab"), I(w2), I(b2), I(d2), dyv(dm), dyv(dr), I(i16(M, C)),
                              O(np.zeros((M, C), np.int16)), M, C, HD], _setup(H, gelu=True))
    for C in (192, 256, 384):
        HD = 4 * C
        lay = [("fc1", _layer(rng, HD, C, 8)), ("fc2", _layer(rng, C, HD, 16))]
        bi, sc, dln = _ln(rng, C)
        lnc = (("bi", bi), ("sc", sc), ("dln", dln))
        for M in (17, 81):                                    # 16-token tiles in units of up to 80 tokens
            # every kernel ivit_mlp_plan_select accepts; "by shape" at width 384 reaches the role-split kernel on a share of one CU
            for sel, cus in ((0, 0), (1, 0)) + (((2, 0), (0, 1)) if C == 384 else ()):
                add("mlp_fused_planned", [R("mlp"), I(i8(M, C)), R("tab"), dyv(dm), dyv(dr), I(i16(M, C)), O(np.zeros((M, C), np.int16)), M],
                    _setup(H, lay, mlp=("fc1", "fc2"), select=sel, cu_share=cus, gelu=True))
            if C != 256:
                add("layernorm_mlp_lockstep_planned", [R("mlp"), I(_x16(rng, M, C)), 2.5e-4, R("bi"), R("sc"), R("dln"), R("tab"), dyv(dm), dyv(dr),
                                                       O(np.zeros((M, C), np.int16)), M], _setup(H, lay, mlp=("fc1", "fc2"), gelu=True, const=lnc))
            if C == 384:
                add("layernorm_mlp_fused_planned", [R("mlp"), I(_x16(rng, M, C)), 2.5e-4, R("bi"), R("sc"), R("dln"), O(np.zeros((M, C), np.int8)), R("tab"),
                                                    dyv(dm), dyv(dr), O(np.zeros((M, C), np.int16)), M],
                    _setup(H, lay, mlp=("fc1", "fc2"), select=2, gelu=True, const=lnc))

    # ---- PatchEmbed in one launch, PatchMerging's gather + norm, the pool with its input scale
    Bp, HW, Dp = 2, 32, 64
    Tp, Kp = (HW // 16) ** 2 + 1, 3 * 256
    w, b, d = _layer(rng, Dp, Kp, 16)
    dx, dp = iv.freeze.dyadic(np.float32(2e-4), np.float32(7e-4)), iv.freeze.dyadic(np.float32(5e-4), np.float32(7e-4))
    add("patch_embed", [I(i8(Bp, 3, HW, HW)), Bp, 3, HW, HW, 16, I(w), I(b), I(d), I(rng.integers(-10 ** 6, 10 ** 6, Dp).astype(np.int32)),
                        I(i16(Tp, Dp)), dyv(dx), dyv(dp), O(np.zeros((Bp * Tp, Dp), np.int16)), Dp])
    for C, Rr in ((96, 14), (192, 6)):
        bi, sc, dln = _ln(rng, 4 * C)
        add("patch_merge_layernorm_requant", [I(i16(2, Rr, Rr, C)), 2, Rr, C, 2.5e-4, I(bi), I(sc), I(dln), O(np.zeros((2 * (Rr // 2) ** 2, 4 * C), np.int8))])
    dpool = iv.freeze.dyadic(np.float32(0.03), np.float32(0.02))
    for L, C in ((144, 256), (49, 96)):                       # even L: rounding ties decided by the fp32 sequence
        add("avgpool_requant_scaled", [I(i8(3, L, C)), 3, L, C, 0.03, dyv(dpool), O(np.zeros((3, C), np.int8))])

    # ---- window attention at window 12: R = 24 (2 x 2 windows) with and without the cyclic shift, R = 12 (one window)
    s12 = np.float32(0.0523)
    d12 = [iv.freeze.dyadic(np.float32(a), np.float32(b)) for a, b in ((0.0021, 0.047), (0.047, s12), (2.0 ** -7 * 0.031, 0.029))]
    for Rr, sh, heads in ((24, 0, 2), (24, 6, 3), (12, 0, 1)):
        add("window_attention_fused", [I(i8(1, Rr, Rr, 3 * heads * 32)), dyv(d12[0]), dyv(d12[1]), I(rng.integers(-40, 41, (heads, 144, 144)).astype(np.int16)),
                                       float(s12), dyv(d12[2]), O(np.zeros((1, Rr * Rr, heads * 32), np.int8)), 1, Rr, 12, sh, heads, 32])

    # ---- top-k: four images per block, so batch 5 leaves a last block with three wavefronts missing; 1000 classes in registers,
    # 1100 rescanned from memory; with and without values
    for ncls, kk, val in ((1000, 5, True), (1100, 16, True), (10, 3, False)):
        add("logits_topk", [I(rng.integers(-2 ** 20, 2 ** 20, (5, ncls)).astype(np.int32)), I(rng.uniform(1e-4, 2e-4, ncls).astype(np.float32)), 5, ncls, kk,
                            O(np.zeros((5, kk), np.int32)), O(np.zeros((5, kk), np.float32)) if val else None])
    return cs


# every prototype of include/ivit.h is in one of the two tables, or here with its reason
EXCLUDED = {
    "version": "returns IVIT_VERSION: no argument",
    "status_string": "status code -> static string: no tensor argument",
    "last_error": "returns the handle's message buffer: no tensor argument",
    "mlp_plan_select": "tuning switch of a plan, a host field: part of the setup of the mlp_fused_planned cases",
    **{n: "tests/test_pil_resize_gpu.py runs them on the arena harness" for n in ("resize_center_crop_u8_pil", "eval_transform_u8")},
    **{n: "plan life cycle, no handle and no tensor argument: the teardown of the planned cases" for n in ("linear_plan_destroy", "mlp_plan_destroy")},
    "linear_plan_query": "query of a plan: writes two host ints",
    **{n: "handle life cycle and settings: no tensor argument" for n in ("create", "destroy", "set_stream", "set_cu_share")},
    **{n: "build-time plan call (allocates, synchronises): the setup of the planned cases" for n in
       ("linear_plan_create", "linear_plan_prepare_ws", "mlp_plan_create")},
    **{n: "host <-> device / RCCL transfer of a whole blob, no kernel of the library" for n in ("constants_upload", "constants_broadcast")},
    **{n: "diagnostic entry of the parity tests" for n in ("debug_div", "debug_requotient")},
    **{n: "hipGraph entry: replays what the runner tests capture" for n in
       ("graph_launch", "graph_destroy", "vit_graph_create", "swin_graph_create", "vit_predict_graph_create", "swin_predict_graph_create")},
    **{n: "whole-model runner: the dirty-workspace tests of tests/test_memory_contract_gpu.py" for n in
       ("vit_create", "vit_destroy", "vit_workspace_bytes", "vit_workspace_init", "vit_forward", "vit_predict",
        "swin_create", "swin_destroy", "swin_workspace_bytes", "swin_forward", "swin_predict")},
    **{n: "query of the runner's launch rule: writes one host int" for n in
       ("vit_fused_mlp_blocks", "vit_fused_ln_mlp_blocks", "vit_fused_qkv_blocks", "vit_cls_tail", "swin_fused_mlp_blocks")},
}


@functools.lru_cache(maxsize=None)
def table_names():
    """(names of _cases, names of hip_cases)"""
    twinned = {n for v in (0, 1) for n, _ in _cases(np.random.default_rng(0), v)}
    return twinned, {c[0] for c in hip_cases(None, np.random.default_rng(0))}


def uncovered_entry_points():
    """prototypes of include/ivit.h that are in neither table and not excluded, and stale exclusions: both must be empty"""
    twinned, hip = table_names()
    every = {n[len("ivit_"):] for n in _lib.ABI.functions}
    return sorted(every - twinned - hip - set(EXCLUDED)), sorted((set(EXCLUDED) - every) | (set(EXCLUDED) & (twinned | hip)))


# ---------------------------------------------------------------- the tables as the contract tests read them: built once, left unchanged
TWIN_SEED, HIP_SEED = 77, 99    # the seeds of the tables every contract test runs
SECOND_SEED = 1234              # a second table of the same cases with other array contents (check_stream_contract, step 5)


@functools.lru_cache(maxsize=None)
def twin_table(variant, seed=TWIN_SEED):
    """_cases of one variant, built once per (variant, seed) and left unchanged (the arenas copy from it)"""
    return _cases(np.random.default_rng(seed + variant), variant)


@functools.lru_cache(maxsize=None)
def hip_table(H, seed=HIP_SEED):
    """the device table, built once per (handle, seed) (None: names and arguments only) and left unchanged"""
    return hip_cases(H, np.random.default_rng(seed))


def cases_of(H, name, second=False):
    """(label, args, setup, twinned) of every case of entry `name` in both tables; second: the tables built from SECOND_SEED — the
    same cases in the same order with other array contents (tests/test_memory_contract_cpu.py::
    test_tables_from_two_seeds_agree_in_everything_but_contents)"""
    out = []
    for variant in (0, 1):
        out += [(f"twinned table, variant {variant}, case {i}", args, None, True)
                for i, (n, args) in enumerate(twin_table(variant, SECOND_SEED if second else TWIN_SEED)) if n == name]
    # a device-table case of a twinned entry goes through the twin as well, unless it sits behind a plan (another handle protocol)
    twinned = name in gen_twin_header.TWIN and name not in NO_TWIN_FORM
    out += [(f"device table, case {i}", args, setup, twinned and (setup is None or not setup.plans))
            for i, (n, args, setup) in enumerate(hip_table(H, SECOND_SEED if second else HIP_SEED)) if n == name]
    return out


def table_differences(a, b):
    """what two argument lists of one case differ in BESIDE the contents of their ("in", ...) arrays -> (list of differences, positions
    of the input arrays whose contents differ, positions of those whose contents are equal)"""
    diffs, changed, same = [], [], []
    if len(a) != len(b):
        return [("length", len(a), len(b))], changed, same
    for i, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, tuple) != isinstance(y, tuple) or (isinstance(x, tuple) and x[0] != y[0]):
            diffs.append((i, "kind"))
        elif not isinstance(x, tuple):
            eq = bytes(x) == bytes(y) if isinstance(x, ctypes.Structure) and type(x) is type(y) else type(x) is type(y) and x == y
            if not eq:
                diffs.append((i, "scalar", x, y))
        elif x[0] in ("ref", "host"):
            if not (np.array_equal(x[1], y[1]) if x[0] == "host" else x[1] == y[1]):
                diffs.append((i, x[0]))
        else:
            if x[1].shape != y[1].shape or x[1].dtype != y[1].dtype or len(x) != len(y):
                diffs.append((i, "shape, dtype or pad", x[1].shape, y[1].shape))
                continue
            if len(x) > 2:
                p, q = x[2], y[2]
                if isinstance(p, tuple) != isinstance(q, tuple) or not (p[0] == q[0] and np.array_equal(p[1], q[1]) if isinstance(p, tuple) else p == q):
                    diffs.append((i, "pad"))
            if x[0] == "in":
                (same if np.array_equal(x[1], y[1]) else changed).append(i)
    return diffs, changed, same


# ---------------------------------------------------------------- arenas: [guard | payload | guard] around every array
GUARD = 1 << 20         # bytes on either side of a payload.  A condition, not a measurement: see _fits
TILE_ROWS = 256         # the tallest row tile of any kernel in the library (gemm_as_kernel's 256-row units)
TILE_ROWS_OF = {"logits_topk": 4}       # entries with long rows and a shorter tile: logits_topk_kernel works four images per block
PAYLOAD_ALIGN = 256     # the payload starts at a multiple of this (plus the shift of an alignment case)


def _fits(a, tile_rows):
    """a kernel that forgets its row mask runs at most one tile past the last row, or one tile in front of the first: the guard
    has to hold (row pitch x tile height) bytes for that store to land in it, and a flat array a whole 1024-thread block of
    16-byte accesses"""
    reach = a.strides[-2] * tile_rows if a.ndim >= 2 else 16 * 1024
    assert reach < GUARD, ("guard too small for", a.shape, a.dtype)


class NumpyMem:
    """host memory: the twin's side"""
    def alloc(self, n):
        buf = np.empty(n, np.uint8)
        return buf, buf.ctypes.data

    def put(self, buf, image):
        buf[:] = image

    def get(self, buf):
        return buf.copy()

    def sync(self):
        pass


class TorchMem:
    """device memory through torch's allocator"""
    def alloc(self, n):
        import torch
        buf = torch.empty(n, dtype=torch.uint8, device="cuda")
        return buf, buf.data_ptr()

    def put(self, buf, image):
        import torch
        buf.copy_(torch.from_numpy(image))

    def get(self, buf):
        return buf.cpu().numpy()

    def sync(self):
        import torch
        torch.cuda.synchronize()


def _valid_mask(arr, pad):
    """boolean byte mask of the payload: True where the bytes are payload proper (inputs: data; outputs: documented as written)"""
    m = np.ones(arr.shape, bool)
    kind = None
    if pad is not None:
        if isinstance(pad, tuple):
            kind, pad = pad
        if kind == "free":
            m = np.asarray(pad, bool).reshape(arr.shape).copy()
        else:
            m[..., pad:] = False
    return np.repeat(m.reshape(-1), arr.itemsize), kind


class Arena:
    """one argument array inside its own allocation; `shift` bytes move the payload off its 256-byte boundary"""
    def __init__(self, mem, arr, is_out, pad=None, shift=0, tile_rows=TILE_ROWS):
        _fits(arr, tile_rows)
        self.mem, self.arr, self.is_out, self.shift = mem, arr, is_out, shift
        self.nbytes = arr.nbytes
        self.valid, self.kind = _valid_mask(arr, pad)
        self.buf, base = mem.alloc(2 * GUARD + self.nbytes + 2 * PAYLOAD_ALIGN)
        self.off = GUARD + (-(base + GUARD)) % PAYLOAD_ALIGN + shift
        self.ptr = _P(base + self.off)
        assert (base + self.off - shift) % PAYLOAD_ALIGN == 0

    def fill(self, byte):
        """outputs: `byte` everywhere.  inputs: `byte` in both guards and in the pad columns (zero where the header demands zero),
        the data in between"""
        img = np.full(2 * GUARD + self.nbytes + 2 * PAYLOAD_ALIGN, byte, np.uint8)
        if not self.is_out:
            pay = np.ascontiguousarray(self.arr).view(np.uint8).reshape(-1).copy()
            pay[~self.valid] = 0 if self.kind == "zero" else byte
            img[self.off:self.off + self.nbytes] = pay
        self.byte = byte
        self.image = img
        self.mem.put(self.buf, img)

    def unchanged(self):
        """the whole allocation still holds what the last fill put there"""
        return np.array_equal(self.mem.get(self.buf), self.image)

    def read(self):
        """-> (payload bytes, number of guard bytes that no longer hold the fill)"""
        img = self.mem.get(self.buf)
        pay = img[self.off:self.off + self.nbytes]
        front, back = img[:self.off], img[self.off + self.nbytes:]
        return pay, int((front != self.byte).sum()), int((back != self.byte).sum())


class ContractError(AssertionError):
    pass


def _place(mem, args, shift_arg=None, tile_rows=TILE_ROWS):
    """an Arena per ("in" | "out", ...) argument, in argument order; shift_arg: index of the one argument moved forward by one element"""
    arenas = []
    for i, a in enumerate(args):
        if isinstance(a, tuple) and a[0] in ("in", "out"):
            pad = a[2] if len(a) > 2 else None
            arenas.append(Arena(mem, a[1], a[0] == "out", pad, a[1].itemsize if i == shift_arg else 0, tile_rows))
    return arenas


def _run_placed(fn, handle, args, arenas, mem, out_fill, in_fill, refs, status=0):
    for ar in arenas:
        ar.fill(out_fill if ar.is_out else in_fill)
    mem.sync()
    queue = iter(arenas)
    _run(fn, handle, args, lambda a, is_out: (next(queue).ptr, None), refs, status)
    mem.sync()
    return [ar.read() for ar in arenas if ar.is_out]


def check_contract(fn, handle, args, mem, refs=None, what="", tile_rows=TILE_ROWS):
    """checks 1 and 2 of the memory contract on one call, -> the output payloads (a list of byte arrays, pads masked to 0):
    1. outputs only: with the output arenas filled 0xA5 and then 0x5A, both guards of every output keep the fill, the bytes an
       entry documents as not written keep it, and every other byte differs from the fill in at least one run;
    2. inputs only: the input guards (and pad columns) hold 0x7F in the first run and 0xFF in the second — NaN as float32, -1
       against 127 as int8 — and the outputs of the two runs are the same bytes."""
    arenas = _place(mem, args, tile_rows=tile_rows)
    runs = [_run_placed(fn, handle, args, arenas, mem, of, inf, refs) for of, inf in ((0xA5, 0x7F), (0x5A, 0xFF))]
    outs = [ar for ar in arenas if ar.is_out]
    res = []
    for i, ar in enumerate(outs):
        (p1, f1, b1), (p2, f2, b2) = runs[0][i], runs[1][i]
        if f1 or f2:
            raise ContractError(f"{what}: output {i} {ar.arr.shape}: {max(f1, f2)} bytes written IN FRONT of the output")
        if b1 or b2:
            raise ContractError(f"{what}: output {i} {ar.arr.shape}: {max(b1, b2)} bytes written BEHIND the output")
        if ar.kind != "free":
            keep = ~ar.valid
            bad = int((p1[keep] != 0xA5).sum() + (p2[keep] != 0x5A).sum())
            if bad:
                raise ContractError(f"{what}: output {i}: {bad} bytes written that the entry documents as not written")
        unwritten = int(((p1 == 0xA5) & (p2 == 0x5A) & ar.valid).sum())
        if unwritten:
            raise ContractError(f"{what}: output {i} {ar.arr.shape}: {unwritten} bytes of the output never written")
        diff = int(((p1 != p2) & ar.valid).sum())
        if diff:
            raise ContractError(f"{what}: output {i} {ar.arr.shape}: {diff} bytes depend on what lies around the inputs")
        res.append(np.where(ar.valid, p1, 0).astype(np.uint8))
    return res


def plain_outputs(fn, handle, args, mem, refs=None):
    """the same call on plain allocations of the exact size -> output payloads in check_contract's form"""
    keep, masks = [], []

    def to_ptr(a, is_out):
        buf, base = mem.alloc(max(a.nbytes, 1))
        mem.put(buf, np.ascontiguousarray(a).view(np.uint8).reshape(-1))
        keep.append(buf)
        return _P(base), buf
    for a in args:
        if isinstance(a, tuple) and a[0] == "out":
            masks.append(_valid_mask(a[1], a[2] if len(a) > 2 else None)[0])
    mem.sync()
    outs = _run(fn, handle, args, to_ptr, refs)
    mem.sync()
    return [np.where(m, mem.get(o), 0).astype(np.uint8) for m, o in zip(masks, outs)]


# ---------------------------------------------------------------- the handle's stream, and a caller's graph
def check_stream_contract(fn, H, args, args2, mem, refs=None, what="", eager_first=True):
    """include/ivit.h, Conventions: every call is asynchronous on the handle's HIP stream, allocates nothing, synchronises nothing and
    is hipGraph-capturable.  One case on plain allocations of the exact size; `args2` is the same argument list with other contents
    in its ("in", ...) arrays; H a _lib.Handle on the current stream.  Every buffer exists before the capture begins, and between
    its begin and its end nothing is allocated and torch is not called.
      1. want1: the eager call on the current stream;
      2. the handle moves to a side stream, the outputs are filled 0x5A, the call is captured there in relaxed mode: IVIT_OK, a graph;
      3. the device is synchronised: every output byte still holds 0x5A (a launch on any stream but the handle's has run by then),
         and the graph holds at least one node;
      4. the graph, instantiated and launched on the side stream, gives want1;
      5. the inputs are overwritten with args2's, the outputs filled 0xA5: the SAME executable graph gives want2, the eager call on
         args2 (a decision taken on the host at call time would be baked into the graph), and the same bytes when launched again.
    eager_first=False leaves step 1 out and takes want1 from an eager call AFTER the first replay: the captured call is then the
    first one the entry sees (tests/first_call_child.py).
    -> (want1, want2), payload bytes in plain_outputs' form.  Raises ContractError with a message per failure mode."""
    import torch
    import hip_runtime
    rt = hip_runtime.bind(H.lib)
    want1 = plain_outputs(fn, H.h, args, mem, refs) if eager_first else None
    ins, outs = [], []
    masks = [_valid_mask(a[1], a[2] if len(a) > 2 else None)[0] for a in args if _is_array(a) and a[0] == "out"]

    def to_ptr(a, is_out):
        buf, base = mem.alloc(max(a.nbytes, 1))
        if is_out:
            outs.append((buf, max(a.nbytes, 1)))
        else:
            mem.put(buf, np.ascontiguousarray(a).view(np.uint8).reshape(-1))
            ins.append(buf)
        return _P(base), None
    call, _ = _marshal(H.h, args, to_ptr, refs)

    def fill(byte):
        for o, n in outs:
            mem.put(o, np.full(n, byte, np.uint8))
        mem.sync()

    def read():
        mem.sync()
        return [mem.get(o) for o, _ in outs]

    def payload(raw):
        return [np.where(m, r[:m.size], 0).astype(np.uint8) for m, r in zip(masks, raw)]

    def differ(got, want):
        return sum(int((g != w).sum()) for g, w in zip(got, want))
    side = torch.cuda.Stream()
    S, graph, gexec = _P(side.cuda_stream), _P(), _P()
    fill(0x5A)
    capturing = False
    try:
        try:
            H.set_stream(side.cuda_stream)
            begun = rt.hipStreamBeginCapture(S, hip_runtime.RELAXED)
            assert begun == 0, f"hipStreamBeginCapture: hipError {begun}"
            capturing = True
            st = fn(*call)
            capturing = False
            ended = rt.hipStreamEndCapture(S, ctypes.byref(graph))
        finally:
            if capturing:                             # the entry raised: leave no stream capturing
                rt.hipStreamEndCapture(S, ctypes.byref(graph))
            H.set_stream(torch.cuda.current_stream().cuda_stream)
        if st != 0:
            raise ContractError(f"{what}: status {st} inside a capture: {H.lib.ivit_last_error(H.h).decode()}")
        if ended != 0 or not graph.value:
            raise ContractError(f"{what}: the capture ended with hipError {ended} and {'a' if graph.value else 'no'} graph")
        for j, raw in enumerate(read()):
            n = int((raw != 0x5A).sum())
            if n:
                raise ContractError(f"{what}: {n} bytes of output {j} written before the graph was launched")
        if rt.node_count(graph) < 1:
            raise ContractError(f"{what}: launched nothing into the capture")
        err = rt.hipGraphInstantiate(ctypes.byref(gexec), graph, None, None, 0)
        assert err == 0 and gexec.value, f"hipGraphInstantiate: hipError {err}"

        def replay():
            err = rt.hipGraphLaunch(gexec, S)
            assert err == 0, f"hipGraphLaunch: hipError {err}"
            return payload(read())
        got = replay()
        if want1 is None:
            want1 = plain_outputs(fn, H.h, args, mem, refs)
        if differ(got, want1):
            raise ContractError(f"{what}: first replay differs from the eager call in {differ(got, want1)} bytes")
        k = 0
        for a in args2:
            if _is_array(a) and a[0] == "in":
                mem.put(ins[k], np.ascontiguousarray(a[1]).view(np.uint8).reshape(-1))
                k += 1
        assert k == len(ins)
        want2 = plain_outputs(fn, H.h, args2, mem, refs)
        fill(0xA5)
        got = replay()
        if differ(got, want2):
            if not differ(got, want1):
                raise ContractError(f"{what}: replay on new inputs gives the old outputs")
            raise ContractError(f"{what}: replay on new inputs differs from the eager call on the new inputs in {differ(got, want2)} bytes")
        again = replay()
        if differ(again, got):
            raise ContractError(f"{what}: second replay of the same inputs differs in {differ(again, got)} bytes")
        return want1, want2
    finally:
        mem.sync()
        if gexec.value:
            rt.hipGraphExecDestroy(gexec)
        if graph.value:
            rt.hipGraphDestroy(graph)


# ---------------------------------------------------------------- alignment of activation pointers
# entry -> {argument index (handle not counted): outcome} for the activation and output pointers of the entry: what happens when that
# ONE pointer is moved forward by one element (data moved with it) to an address that is no multiple of 16.
#   "exact"             same bytes as the aligned call: the kernels touch the pointer with element-sized accesses only
#   ("refused", word)   IVIT_ERR_INVALID before anything is launched, ivit_last_error contains `word`, the outputs keep their fill
# Filled in from the launchers (csrc/ivit_hip.hip) and the kernels they start, not from runs: see the comment at each group.
def _a16(name):
    return ("refused", name + " must be 16-byte aligned")


_EX = "exact"
_CLS = ("refused", "ctx_cls, x16 and x_cls must be 16-byte aligned")
_TOK = ("refused", "x, out, bias_int, sc must be 16-byte aligned")
_GATHER = ("refused", "x and out 16-byte aligned")
ALIGN = {
    # byte-wise kernels (normalize_quantize_u8_kernel, resize_h_kernel / resize_v_kernel), one element per lane and access
    # (shiftmax_kernel, shiftmax_masked_kernel, requant_bcast_kernel, avgpool_requant_kernel, layernorm_tokenorder_kernel,
    # widen_i8_i16_kernel, logits_topk_kernel): nothing wider than the element ever touches the pointer
    "normalize_quantize_u8": {0: _EX, 7: _EX}, "resize_center_crop_u8": {0: _EX, 7: _EX},
    "shiftmax": {0: _EX, 6: _EX}, "shiftmax_masked": {0: _EX, 9: _EX}, "requant_i32_bcast": {0: _EX, 6: _EX},
    "avgpool_requant": {0: _EX, 5: _EX}, "avgpool_requant_scaled": {0: _EX, 6: _EX}, "layernorm_tokenorder": {0: _EX, 7: _EX},
    "widen_i8_i16": {0: _EX, 1: _EX}, "logits_topk": {0: _EX, 5: _EX, 6: _EX},
    # requant_any: z and z_id are read element by element in both kernels; an output off its 16-byte boundary takes
    # requant_kernel (one element per store) instead of requant_vec8_kernel (8- and 16-byte stores)
    "requant_i32": {0: _EX, 3: _EX, 6: _EX}, "requant_i16": {0: _EX, 3: _EX, 6: _EX}, "requant_f32": {0: _EX, 3: _EX, 6: _EX},
    # quantize_input_kernel: four floats per load (v4f), four packed bytes per store
    "quantize_input_f32": {0: _a16("x"), 2: ("refused", "q must be 4-byte aligned")},
    # the GEMMs stage A and B rows in 16-byte chunks (load_chunk_i8, the LDS-DMA of gemm_glds_kernel, gemm_ps / gemm_as / gemm_ws /
    # gemm_wreg_kernel) and write 8- and 16-bit tiles, q, k and row-major v in 16-byte stores; v^T is stored byte by byte but shares
    # the argument with row-major v.  The int32 accumulators of gemm_nt_kernel (EPI_RAW32) are stored one by one: the runners' head
    # GEMM writes logits + b0 * num_classes of a slice, any multiple of 4
    "linear_i8": {0: _a16("x"), 3: _EX}, "bmm_nt_i8": {0: _a16("A"), 1: _a16("B"), 2: _EX}, "bmm_nt_u16i8": {0: _a16("A"), 1: _a16("B"), 2: _EX},
    "linear_i8_requant": {0: _a16("x"), 5: _a16("out")}, "linear_i8_requant8_store16": {0: _a16("x"), 4: _a16("out16")},
    "linear_i8_requant_residual": {0: _a16("x"), 6: _a16("residual"), 7: _a16("out")},
    "linear_i8_qkv": {0: _a16("x"), 4: _a16("q"), 5: _a16("k"), 6: _a16("vt")},
    "attn_qk_requant": {0: _a16("q"), 1: _a16("k"), 3: _a16("scores8")}, "attn_pv_requant": {0: _a16("p"), 1: _a16("vt"), 3: _a16("ctx8")},
    "linear_i8_requant_planned": {1: _a16("x"), 3: _a16("out")},
    "linear_i8_requant_residual_planned": {1: _a16("x"), 4: _a16("residual"), 5: _a16("out")},
    "layernorm_linear_i8_requant_planned": {1: _a16("x16"), 6: _a16("out8")},
    "linear_i8_requant_residual_layernorm_planned": {1: _a16("x"), 4: _a16("residual"), 5: _a16("out"), 11: _a16("ln_out8")},
    "linear_i8_qkv_planned": {1: _a16("x"), 2: _a16("q"), 3: _a16("k"), 4: _a16("vt")},
    "layernorm_linear_i8_qkv_planned": {1: _a16("x16"), 6: _a16("q"), 7: _a16("k"), 8: _a16("vt")},
    "layernorm_linear_i8_qkv_ldv_planned": {1: _a16("x16"), 6: _a16("q"), 7: _a16("k"), 8: _a16("vt")},
    "patch_embed": {0: _a16("images"), 13: _a16("x16")},
    # attn_fused_kernel stages q, k and v in 16-byte pieces and stores 16 context bytes per lane; the class-token forms already
    # refused ctx_cls, x16 and x_cls (one check, one message)
    "attention_fused": {0: _a16("q"), 1: _a16("k"), 2: _a16("vt"), 6: _a16("ctx8")},
    "attention_fused_lut": {0: _a16("q"), 1: _a16("k"), 2: _a16("vt"), 12: _a16("ctx8")},
    "attention_fused_rowlut": {0: _a16("q"), 1: _a16("k"), 2: _a16("vt"), 8: _a16("ctx8")},
    "attention_fused_cls": {0: _a16("q"), 1: _a16("k"), 2: _a16("vt"), 6: _CLS, 7: _CLS, 8: _CLS},
    "attention_fused_lut_cls": {0: _a16("q"), 1: _a16("k"), 2: _a16("vt"), 12: _CLS, 13: _CLS, 14: _CLS},
    "attention_fused_rowlut_cls": {0: _a16("q"), 1: _a16("k"), 2: _a16("vt"), 8: _CLS, 9: _CLS, 10: _CLS},
    "gather_rows_i16": {0: _GATHER, 4: _GATHER},
    "window_attention_fused": {0: _a16("qkv"), 6: _a16("ctx")}, "window_attention_fused_lut": {0: _a16("qkv"), 12: _a16("ctx")},
    # row kernels with 16 bytes (8 for the 8-bit outputs of the LayerNorms) per lane: shiftgelu_kernel, shiftgelu_lut2_kernel,
    # layernorm_kernel / layernorm16_kernel / layernorm_reg_kernel, im2col_patch16_kernel, embed_finish_kernel,
    # patch_merge_gather_kernel (8 input bytes per lane at 8 bits), layernorm_tokenorder8_kernel (refused before this table)
    "shiftgelu": {0: _a16("x"), 4: _a16("out16")}, "shiftgelu_requant": {0: _a16("x"), 5: _a16("out8")},
    "shiftgelu_requant_lut": {0: _a16("x"), 4: _a16("out8")},
    "layernorm": {0: _a16("x"), 6: _a16("z")}, "layernorm_requant": {0: _a16("x"), 8: _a16("out8")},
    "patch_merge_layernorm_requant": {0: _a16("x"), 8: _a16("out8")},
    "im2col_patch": {0: _a16("img"), 6: _a16("rows")}, "embed_finish": {0: _a16("patch16"), 5: _a16("x16")},
    "patch_merge_gather": {0: ("refused", "x must be "), 5: _a16("out")},
    "layernorm_tokenorder_requant": {0: _TOK, 8: _TOK}, "patch_norm_tokenorder": {0: _TOK, 9: _TOK},
    # the fused Mlp kernels read activation and identity rows and store output rows in 16-byte pieces (8 at C = 128: residual, out)
    "mlp_fused": {0: _a16("x"), 10: ("refused", "residual must be "), 11: ("refused", "out must be ")},
    "mlp_fused_planned": {1: _a16("x"), 5: _a16("residual"), 6: _a16("out")},
    "layernorm_mlp_fused_planned": {1: _a16("x16"), 6: _a16("scratch8"), 10: _a16("out")},
    "layernorm_mlp_lockstep_planned": {1: _a16("x16"), 9: _a16("out")},
}


# twinned entries whose device-table cases the twin has no form for: ivit_cpu_window_attention_fused is written for window 7 alone
# (oracle/ivit_twin.c), the device table holds the window-12 cases
NO_TWIN_FORM = {"window_attention_fused"}

# entries whose only arrays are tables (built once per frozen layer, 256-byte aligned in the constants blob): no activation pointer
TABLES_ONLY = {"shiftgelu_build_table", "shiftmax_rowtable"}


def alignment_table_gaps():
    """(entries with a case that holds an ("in" | "out") array but are in neither ALIGN nor TABLES_ONLY; ALIGN records that name no
    entry with a case, or an index that is not an array argument in every case of the entry): both must be empty"""
    cases = [(n, a) for v in (0, 1) for n, a in _cases(np.random.default_rng(0), v)] + [(n, a) for n, a, _ in hip_cases(None, np.random.default_rng(0))]
    is_array = lambda a: isinstance(a, tuple) and a[0] in ("in", "out")
    missing = sorted({n for n, args in cases if any(is_array(a) for a in args)} - set(ALIGN) - TABLES_ONLY)
    wrong = [(n, idx) for n, spec in ALIGN.items() for idx in spec
             if not any(c == n for c, _ in cases) or any(not (args[idx] is None or is_array(args[idx])) for c, args in cases if c == n)]
    return missing, wrong + sorted(TABLES_ONLY & set(ALIGN))


def check_alignment(fn, H, args, mem, refs, idx, outcome, aligned, what, tile_rows=TILE_ROWS):
    """check 4: the call with argument `idx` one element off its 256-byte boundary, against the recorded outcome; `aligned` are the
    output payloads of the aligned call (check_contract's result)"""
    arenas = _place(mem, args, shift_arg=idx, tile_rows=tile_rows)
    assert arenas and any(ar.shift for ar in arenas) and all(ar.ptr.value % 16 for ar in arenas if ar.shift)
    what = f"{what}, argument {idx} one element off its 16-byte boundary"
    if outcome == "exact":
        outs = _run_placed(fn, H.h, args, arenas, mem, 0xA5, 0x7F, refs)
        for i, (ar, (pay, front, back)) in enumerate(zip([a for a in arenas if a.is_out], outs)):
            if front or back:
                raise ContractError(f"{what}: output {i}: {front} bytes written in front of, {back} behind the output")
            got = np.where(ar.valid, pay, 0).astype(np.uint8)
            if not np.array_equal(got, aligned[i]):
                raise ContractError(f"{what}: output {i}: {int((got != aligned[i]).sum())} bytes differ from the aligned call")
            if ar.kind != "free" and (pay[~ar.valid] != 0xA5).any():
                raise ContractError(f"{what}: output {i}: bytes written that the entry documents as not written")
        return
    kind, word = outcome
    assert kind == "refused"
    outs = _run_placed(fn, H.h, args, arenas, mem, 0xA5, 0x7F, refs, status=_lib.IVIT_ERR_INVALID)
    msg = H.lib.ivit_last_error(H.h).decode()
    if word not in msg or "aligned" not in msg:
        raise ContractError(f"{what}: refused, but not with the message {word!r}: {msg!r}")
    for i, (pay, front, back) in enumerate(outs):
        if front or back or (pay != 0xA5).any():
            raise ContractError(f"{what}: refused, but output {i} was written")


# ---------------------------------------------------------------- overlapping arguments
# include/ivit.h, "overlapping arguments": an array an entry writes (an ("out", ...) argument, scratch included) may overlap neither an
# activation input (the ("in", ...) arguments ALIGN lists) nor another array the entry writes; the call is refused with
# IVIT_ERR_INVALID before anything is launched.  INPLACE lists the exceptions: entry -> {(input index, output index): reason}, indices
# as in ALIGN — the same pointer with the same extent is accepted and gives the bytes of the call on disjoint arrays.  Everything not
# listed is refused.  Filled in from the kernels every launcher can start (csrc/ivit_hip.hip), not from runs; a pair is listed only if
# every element of the input is loaded only by the lane that stores it, before that store, in every one of those kernels.
INPLACE = {
    # gemm_nt_kernel, gemm_glds_kernel: the epilogue lane of (grow, gcol) loads eight identity values under the same grow < M,
    # gcol < N test as its store of those eight elements, the load first.  gemm_wreg_kernel: a lane loads the identity of its own row
    # and channels ahead of the MFMAs and stores those elements behind them; a lane past M loads row M - 1 but every store is under
    # `live`, so that value reaches no store.  All three take a GemmArgs by value: no pointer is declared __restrict__.
    # Cases: the twinned table at M = 300 and 173 (gemm_glds_kernel<EPI, 128>, 3 and 2 row tiles; the 256-row instantiation is
    # reached by no call at all: tests/test_memory_contract_cpu.py::test_glds_256_row_tile_is_unreachable), M = 8209
    # (gemm_wreg_kernel), M = 257 at K = 48 (gemm_nt_kernel, 3 row tiles).
    # The PLANNED form stays refused: gemm_ps_kernel / gemm_as_kernel request identity pieces asynchronously rounds ahead of the
    # epilogue at offsets clamped for rows past M, gemm_ws_qkv_kernel reads row min(row, M - 1); their order against the stores of the
    # owning lanes is not established, and the launcher picks among five kernels by shape.
    "linear_i8_requant_residual": {(6, 7): "residual == out: each epilogue lane loads exactly the identity elements it stores, load first"},
}
# Decided the other way, by the same reading:
#   requant_i16 (z == out at 16 bits), shiftgelu_requant (x == out8), shiftgelu_requant_lut: requant_kernel, requant_vec8_kernel,
#     shiftgelu_kernel and the shiftgelu_lut kernels declare input and output __restrict__; lane by lane each element is loaded only by
#     the lane that stores it, but aliasing two __restrict__ pointers is undefined whatever the lanes do, and no kernel changes here;
#   mlp_fused (swin_mlp_fused_kernel, swin_mlp_rs_kernel, mlp128_kernel), mlp_fused_planned (mlp192 / mlp256 / mlp384_kernel,
#     mlp384rs_kernel): the identity of rows past M - 1 of a tile is row M - 1 (min(tok, M - 1)), which another tile's lanes store, and
#     in the role-split kernels the identity is loaded by consumer waves while producer waves of the same workgroup are a unit ahead;
#   layernorm_mlp_fused_planned: x16 is fetched twice (LayerNorm head, identity branch) by different lanes at different times;
#   layernorm_mlp_lockstep_planned, linear_i8_requant_residual_layernorm_planned: fixed (the latter re-reads `out` through L1).
ALWAYS_REFUSED = ("layernorm_mlp_lockstep_planned", "linear_i8_requant_residual_layernorm_planned")


def _is_array(a):
    return isinstance(a, tuple) and a[0] in ("in", "out")


def overlap_pairs(name, args, inputs=None):
    """[(first index, second index)] of one case: every (activation input, output) and every (output, output) pair; the activation
    inputs are the ones ALIGN lists for the entry (`inputs`: given instead, for an entry that is in no table)"""
    ins = [i for i in sorted(ALIGN.get(name, {}) if inputs is None else inputs) if _is_array(args[i]) and args[i][0] == "in"]
    outs = [i for i, a in enumerate(args) if _is_array(a) and a[0] == "out"]
    return [(i, o) for i in ins for o in outs] + [(o1, o2) for k, o1 in enumerate(outs) for o2 in outs[k + 1:]]


def overlap_table_gaps():
    """records of INPLACE that name no entry with a case, an input that is no activation input or an output that is no output of every
    case, arrays of different size, or an entry that is refused by decree: must be empty"""
    cases = [(n, a) for v in (0, 1) for n, a in _cases(np.random.default_rng(0), v)] + [(n, a) for n, a, _ in hip_cases(None, np.random.default_rng(0))]
    wrong = []
    for name, pairs in INPLACE.items():
        mine = [args for n, args in cases if n == name]
        if not mine or name in ALWAYS_REFUSED:
            wrong.append((name, "no case / refused by decree"))
        for (i, o), reason in pairs.items():
            ok = reason and i in ALIGN.get(name, {}) and all(
                _is_array(args[i]) and args[i][0] == "in" and _is_array(args[o]) and args[o][0] == "out" and args[i][1].nbytes == args[o][1].nbytes
                for args in mine)
            if not ok:
                wrong.append((name, i, o))
    return wrong


def _r256(n):
    return (n + 255) // 256 * 256


def overlap_placements(na, nb):
    """{placement: (offset of a, offset of b)} of two arrays of na and nb bytes; all offsets multiples of 256 (16 inside a short a)"""
    pl = {"same start": (0, 0), "b begins inside a": (0, 256 if na >= 512 else 16)}
    back = 256 * ((nb - 1) // 256)
    if back:
        pl["b ends inside a"] = (back, 0)
    pl["b behind a"] = (0, _r256(na))
    pl["a behind b"] = (_r256(nb), 0)
    return pl


class _Shared:
    """two argument arrays in ONE allocation, at byte offsets `offs` from a 256-byte boundary, with the 1 MiB guards on both sides of
    their union: a call that is wrongly not refused still addresses only this allocation"""
    def __init__(self, mem, specs, offs, tile_rows):
        self.mem, self.specs = mem, specs                 # specs: [(is_out, array, valid mask, kind)]
        for _, arr, _, _ in specs:
            _fits(arr, tile_rows)
        span = max(o + s[1].nbytes for o, s in zip(offs, specs))
        self.size = 2 * GUARD + span + 2 * PAYLOAD_ALIGN
        self.buf, base = mem.alloc(self.size)
        origin = GUARD + (-(base + GUARD)) % PAYLOAD_ALIGN
        self.off = [origin + o for o in offs]
        self.ptr = [_P(base + o) for o in self.off]
        assert min(self.off) >= GUARD and max(o + s[1].nbytes for o, s in zip(self.off, specs)) + GUARD <= self.size

    def fill(self, out_fill, in_fill):
        img = np.full(self.size, in_fill, np.uint8)
        for off, (is_out, arr, _, _) in zip(self.off, self.specs):
            if is_out:
                img[off:off + arr.nbytes] = out_fill
        for off, (is_out, arr, valid, kind) in zip(self.off, self.specs):       # the data last: an input under an output keeps it
            if not is_out:
                pay = np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()
                pay[~valid] = 0 if kind == "zero" else in_fill
                img[off:off + arr.nbytes] = pay
        self.image = img
        self.mem.put(self.buf, img)


def check_overlap(fn, H, args, mem, refs, what, tile_rows=TILE_ROWS, name=None, inplace=None, inputs=None, argnames=None):
    """the overlap contract on one case: every pair of overlap_pairs in every placement of overlap_placements, inside one shared
    allocation.  An overlapping placement is refused (IVIT_ERR_INVALID, `overlap` in the message, no byte of any arena changed) unless
    it is the same start of an INPLACE pair of equal size: that one runs twice and gives the bytes of the plain call both times.  The
    adjacent placements succeed with the bytes of the plain call, which keeps an entry from over-estimating an extent.
    H: the handle object (H.h, H.lib.ivit_last_error); name: the entry (its INPLACE record, unless `inplace` is given);
    argnames: the entry's parameter names as the header spells them, handle not counted (default: include/ivit.h's, by `name`) — a
    refusal names both arguments of the pair"""
    inplace = INPLACE.get(name, {}) if inplace is None else inplace
    if argnames is None and name is not None:
        argnames = [p.name for p in _lib.ABI.functions["ivit_" + name].params[1:]]
    want = plain_outputs(fn, H.h, args, mem, refs)
    arr_idx = [i for i, a in enumerate(args) if _is_array(a)]
    out_rank = {i: k for k, i in enumerate(i for i in arr_idx if args[i][0] == "out")}
    spec = {i: (args[i][0] == "out", args[i][1]) + _valid_mask(args[i][1], args[i][2] if len(args[i]) > 2 else None) for i in arr_idx}
    own = {i: Arena(mem, args[i][1], args[i][0] == "out", args[i][2] if len(args[i]) > 2 else None, 0, tile_rows) for i in arr_idx}

    def verify(sh, pair, others, ran, label):
        """ran: the call was to succeed.  Outputs hold `want` where the entry documents a write; nothing else changed anywhere"""
        mem.sync()
        img = mem.get(sh.buf)
        allowed = np.zeros(sh.size, bool)
        for off, idx in zip(sh.off, pair):
            is_out, arr, valid, kind = spec[idx]
            if is_out and ran:
                got = img[off:off + arr.nbytes]
                if not np.array_equal(np.where(valid, got, 0), want[out_rank[idx]]):
                    raise ContractError(f"{label}: argument {idx}: {int((np.where(valid, got, 0) != want[out_rank[idx]]).sum())} bytes differ from the call on disjoint arrays")
                allowed[off:off + arr.nbytes] |= (valid if kind != "free" else True)
        bad = int(((img != sh.image) & ~allowed).sum())
        if bad:
            raise ContractError(f"{label}: {bad} bytes changed in the shared allocation outside what the entry documents as written")
        for idx in others:
            ar = own[idx]
            if ar.is_out and ran:
                pay, front, back = ar.read()
                if front or back or not np.array_equal(np.where(ar.valid, pay, 0), want[out_rank[idx]]):
                    raise ContractError(f"{label}: output argument {idx} differs from the call on disjoint arrays, or its guards changed")
                if ar.kind != "free" and (pay[~ar.valid] != ar.byte).any():
                    raise ContractError(f"{label}: output argument {idx}: bytes written that the entry documents as not written")
            elif not ar.unchanged():
                raise ContractError(f"{label}: argument {idx}, which is not part of the pair, was written")

    for a, b in overlap_pairs(name, args, inputs):
        na, nb = args[a][1].nbytes, args[b][1].nbytes
        others = [i for i in arr_idx if i not in (a, b)]
        for place, (oa, ob) in overlap_placements(na, nb).items():
            label = f"{what}, arguments {a} and {b}, {place}"
            overlapping = oa < ob + nb and ob < oa + na
            assert overlapping == (place in ("same start", "b begins inside a", "b ends inside a")), label
            in_place = place == "same start" and na == nb and (a, b) in inplace
            sh = _Shared(mem, [spec[a], spec[b]], (oa, ob), tile_rows)
            ptr = {a: sh.ptr[0], b: sh.ptr[1], **{i: own[i].ptr for i in others}}
            for run in range(2 if in_place else 1):
                sh.fill(0xA5, 0x7F)
                for i in others:
                    own[i].fill(0xA5 if own[i].is_out else 0x7F)
                mem.sync()
                queue = iter(arr_idx)
                ran = in_place or not overlapping
                try:
                    _run(fn, H.h, args, lambda arr, is_out: (ptr[next(queue)], None), refs, 0 if ran else _lib.IVIT_ERR_INVALID)
                except AssertionError as e:
                    mem.sync()
                    raise ContractError(f"{label}: status {e.args[0] if e.args else '?'}, expected {'IVIT_OK' if ran else 'IVIT_ERR_INVALID (not refused)'}"
                                        f"{'' if overlapping else ': ' + H.lib.ivit_last_error(H.h).decode()}") from None
                if not ran:
                    msg = H.lib.ivit_last_error(H.h).decode()
                    if "overlap" not in msg:
                        raise ContractError(f"{label}: refused, but not with a message about the overlap: {msg!r}")
                    if argnames and not (argnames[a] in msg and argnames[b] in msg):
                        raise ContractError(f"{label}: refused, but the message does not name {argnames[a]} and {argnames[b]}: {msg!r}")
                verify(sh, (a, b), others, ran, label + (f", run {run + 1}" if in_place else ""))
