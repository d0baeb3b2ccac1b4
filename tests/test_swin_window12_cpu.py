"""Swin with a 12 x 12 window (SwinTransformer(window_size=12): the patch4_window12_384 family) on the CPU side:
the oracle against the reference's fixtures up to the pool, and the pool's fp32 sequence at an even token count
(L = 144), restated with torch's own reduction — the order ivit_avgpool_requant_scaled follows.  CPU only."""
import hashlib

import numpy as np
import pytest
import torch

from conftest import load_golden, golden_scales, csum
import ivit_amd as iv
from oracle import oracle as orc

FIXTURES = ["micro_swin_w12_b2.npz", "swin_base_384_b1.npz"]


def _digest(w):
    h = hashlib.sha256()
    for k in sorted(w):
        h.update(k.encode())
        h.update(np.ascontiguousarray(w[k]).tobytes())
    return h.hexdigest()


def _dy(s_in, s_out):
    d = orc.dyadic(np.float32(s_in), np.float32(s_out))
    return float(d[0].m) * float(d[0].r)


def torch_pool_requant(q, s, s_out):
    """AdaptiveAvgPool1d(1) over tokens + QuantAct(8) as the reference computes it: X = fl(Q*s), torch's token sum,
    fl(sum/L), rint(fl(mean/s)), then the dyadic requant of the next QuantAct.  q: int8 [B, L, C]."""
    X = torch.from_numpy(q.astype(np.float32)) * torch.tensor(np.float32(s))
    mean = torch.sum(X, dim=1) / q.shape[1]
    z = torch.round(mean / torch.tensor(np.float32(s))).numpy().astype(np.float64)
    return np.clip(np.rint(z * _dy(s, s_out)), -128, 127).astype(np.int32)


def cascade_pool_z(q, s):
    """The kernel's restatement (ivit_swin.h avgpool_requant_kernel, even L): per channel a sequential fp32 sum over
    tokens with the 16-step cascade, fl(sum/L), rint(fl(mean/s))."""
    B, L, C = q.shape
    X = q.astype(np.float32) * np.float32(s)
    z = np.empty((B, C), np.float64)
    for b in range(B):
        for c in range(C):
            a = [np.float32(0)] * 4
            i = 0
            while i + 16 <= L:
                for _ in range(16):
                    a[0] = np.float32(a[0] + X[b, i, c])
                    i += 1
                a[1] = np.float32(a[1] + a[0]); a[0] = np.float32(0)
                if i & 0xF0:
                    continue
                a[2] = np.float32(a[2] + a[1]); a[1] = np.float32(0)
                if i & 0xF00:
                    continue
                a[3] = np.float32(a[3] + a[2]); a[2] = np.float32(0)
            while i < L:
                a[0] = np.float32(a[0] + X[b, i, c])
                i += 1
            t = np.float32(np.float32(a[0] + a[1]) + a[2])
            t = np.float32(t + a[3])
            mean = np.float32(t / np.float32(L))
            z[b, c] = np.rint(np.float32(mean / np.float32(s)))
    return z


def tie_block(B, L, C, seed):
    """int8 [B, L, C] whose every channel sums to 72 mod 144 (L = 144): the exact mean sits on a rounding tie."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-100, 101, (B, L, C)).astype(np.int64)
    part = q[:, :-1, :].sum(axis=1)
    r = (L // 2 - part) % L
    q[:, -1, :] = np.where(r > 127, r - L, r)
    assert ((q.sum(axis=1) % L) == L // 2).all()
    return q.astype(np.int8)


def _oracle_run(fname):
    g = load_golden(fname)
    cfg = iv.SWIN_CONFIGS[str(g["cfg_name"])]
    assert cfg.window_size == 12
    w = iv.make_swin_weights(cfg, int(g["seed"]))
    assert _digest(w) == str(g["weights_sha256"])
    o = orc.OracleSwin(cfg, w, golden_scales(g))
    cap = {}
    o.forward(iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"])), cap)
    return g, cfg, o, cap


@pytest.mark.parametrize("fname", FIXTURES)
def test_oracle_reproduces_window12_fixture_before_the_pool(fname):
    """OracleSwin at window 12 (shift 6, masks over 144-token windows, rel-pos bias of 23 x 23) equals the reference at
    every captured site before qact3 (the pool, whose oracle sum order is not the reference's at even L)."""
    g, cfg, o, cap = _oracle_run(fname)
    sites = [str(n) for n in g["sites"]]
    assert sites[-2:] == ["qact3", "head"]
    for n in sites[:-2]:
        v = cap[n]
        if "norm" in n.split(".")[-1]:
            v = np.asarray(v, np.float64)
        assert csum(v) == g["csum/" + n], n


@pytest.mark.parametrize("fname", FIXTURES)
def test_torch_pool_restatement_reproduces_qact3_and_logits(fname):
    """torch's pool (sum over dim 1, / L, rint, dyadic requant) on the oracle's qact2 gives the reference's qact3, and
    the head on it the reference's int32 logits; the kernel's cascade restatement gives the same integers."""
    g, cfg, o, cap = _oracle_run(fname)
    sc = golden_scales(g)
    a = np.asarray(cap["qact2"]).astype(np.int8)
    B = int(g["batch"])
    a = a.reshape(B, -1, a.shape[-1])
    assert a.shape[1] == 144
    pooled = torch_pool_requant(a, sc["qact2"], sc["qact3"])
    assert csum(pooled) == g["csum/qact3"]
    z = cascade_pool_z(a, sc["qact2"])
    assert np.array_equal(np.clip(np.rint(z * _dy(sc["qact2"], sc["qact3"])), -128, 127).astype(np.int32), pooled)
    w_int, b_int, _, _ = o._lin("head", sc["qact3"], None)
    logits = orc.linear_i8(pooled.astype(np.int8), w_int, b_int)
    assert np.array_equal(logits, g["logits_int"])


def test_cascade_restatement_equals_torch_sum_order():
    """The kernel's per-channel cascade equals torch's sum over the token dim bit for bit (L = 144 and L = 49)."""
    rng = np.random.default_rng(3)
    for L in (144, 49):
        q = rng.integers(-128, 128, (2, L, 96)).astype(np.int8)
        s = np.float32(0.0371)
        X = torch.from_numpy(q.astype(np.float32)) * torch.tensor(s)
        ref = torch.round((torch.sum(X, dim=1) / L) / torch.tensor(s)).numpy()
        assert np.array_equal(cascade_pool_z(q, s), ref.astype(np.float64)), L


def test_tie_block_defeats_the_integer_shortcut():
    """On a block whose channel sums are all 72 mod 144 the integer shortcut rint(sum(Q)/L) disagrees with the
    reference's fp32 pool on some channels — so a GPU pool test on this block can fail."""
    q = tie_block(2, 144, 256, seed=5)
    s, s_out = np.float32(0.0417), np.float32(0.0213)
    ref = torch_pool_requant(q, s, s_out)
    z_int = np.rint(q.astype(np.int64).sum(axis=1) / 144.0)
    old = np.clip(np.rint(z_int * _dy(s, s_out)), -128, 127).astype(np.int32)
    assert (old != ref).sum() >= 1
    assert np.array_equal(np.clip(np.rint(cascade_pool_z(q, s) * _dy(s, s_out)), -128, 127).astype(np.int32), ref)


def test_window12_configs_and_factory():
    from ivit_amd import swin_quant
    m = iv.SWIN_CONFIGS["micro_swin_w12"]
    assert (m.img_size, m.embed_dim, m.depths, m.num_heads, m.window_size, m.num_classes) == (96, 32, (2, 2), (1, 2), 12, 10)
    b = iv.SWIN_CONFIGS["swin_base_384"]
    assert (b.img_size, b.embed_dim, b.depths, b.num_heads, b.window_size) == (384, 128, (2, 2, 18, 2), (4, 8, 16, 32), 12)
    assert "no factory" in swin_quant.swin_base_patch4_window12_384.__doc__     # the reference's factories fix window 7
    assert iv.swin_base_patch4_window12_384 is swin_quant.swin_base_patch4_window12_384


def test_engine_window_guard():
    """check_swin_windows: windows 7 and 12 (stage resolutions multiples of the window, or at most it) pass; others
    raise IvitError."""
    from ivit_amd import _lib
    from ivit_amd.swin_engine import check_swin_windows
    for name in ("micro_swin", "swin_tiny", "swin_base", "micro_swin_w12", "swin_base_384"):
        check_swin_windows(iv.SWIN_CONFIGS[name])
    for ws, img in ((8, 128), (6, 96), (12, 224)):
        cfg = iv.SwinConfig("bad", img_size=img, num_classes=10, embed_dim=32, depths=(2, 2), num_heads=(1, 2),
                            window_size=ws)
        with pytest.raises(_lib.IvitError):
            check_swin_windows(cfg)


def test_order_sensitive_shiftmax_rows():
    """The fixture rows (tools/make_shiftmax_order_rows.py): the host restatement with torch's n = 144 order equals the
    oracle's Shiftmax, and a sequential row sum gives different probabilities on every row — so a window-12 kernel that
    summed in another order fails the GPU test built on them."""
    from shiftmax144 import exps, probs, sum_a7, sum_seq
    g = load_golden("shiftmax144_order_rows.npz")
    rows, s = g["rows"], np.float32(g["scale"])
    e = exps(rows, s)
    assert np.array_equal(probs(e, sum_a7(e)), orc.shiftmax(rows, s, 8).astype(np.int32))
    assert (probs(e, sum_a7(e)) != probs(e, sum_seq(e))).any(axis=1).all()
