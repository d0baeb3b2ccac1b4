"""Host restatement of the 8-bit Shiftmax over 144-wide rows (window 12) with a choice of row-sum order: torch's
(SURVEY A.7 for n = 144, what the oracle and window_attention12_kernel use) or a plain sequential sum.  fp32 throughout,
one rounding per operation, as oracle/ivit_oracle.c iexp_shift / ivit_ref_shiftmax."""
import numpy as np

f32 = np.float32


def exps(a, s):
    """exp_int of int8 rows a [..., 144] at scale s (x = fl(fl(a*s)/s) - max, shift-exp with n = 15)"""
    s = f32(s)
    xt = ((a.astype(f32) * s).astype(f32) / s).astype(f32)
    x = (xt - xt.max(axis=-1, keepdims=True)).astype(f32)
    x0 = f32(np.floor(f32(-1.0) / s))
    t = (x + np.floor(x / f32(2))).astype(f32)
    t = np.maximum((t - np.floor(x / f32(16))).astype(f32), f32(15.0) * x0)
    q = np.floor(t / x0).astype(f32)
    r = (t - (x0 * q).astype(f32)).astype(f32)
    e = ((r / f32(2)).astype(f32) - x0).astype(f32)
    e = np.floor((e * np.ldexp(f32(1), (15 - q).astype(np.int32)).astype(f32)).astype(f32))
    return np.maximum(e, f32(0))


def sum_a7(e):
    """torch's order for n = 144: accumulators sub = k mod 32 over keys sub, 32+sub, 64+sub, 96+sub (then 128+sub and
    136+sub for sub < 8), p[l] = ((a[l] + a[8+l]) + a[16+l]) + a[24+l], S = p[0] + ... + p[7]"""
    e = e.reshape(-1, 144)
    acc = (((e[:, 0:32] + e[:, 32:64]).astype(f32) + e[:, 64:96]).astype(f32) + e[:, 96:128]).astype(f32)
    acc[:, :8] = ((acc[:, :8] + e[:, 128:136]).astype(f32) + e[:, 136:144]).astype(f32)
    p = (((acc[:, 0:8] + acc[:, 8:16]).astype(f32) + acc[:, 16:24]).astype(f32) + acc[:, 24:32]).astype(f32)
    S = p[:, 0].copy()
    for l in range(1, 8):
        S = (S + p[:, l]).astype(f32)
    return S


def sum_seq(e):
    e = e.reshape(-1, 144)
    S = e[:, 0].copy()
    for j in range(1, 144):
        S = (S + e[:, j]).astype(f32)
    return S


def probs(e, S):
    """8-bit probabilities: F = floor(fl(1/S) * 2^31), P = floor(fl(e * F) / 2^24)"""
    e = e.reshape(-1, 144)
    F = np.floor((f32(1) / np.minimum(S, f32(2147483648.0))).astype(f32) * f32(2147483648.0)).astype(f32)
    return np.floor((e * F[:, None]).astype(f32) / f32(2 ** 24)).astype(np.int32)
