"""Swin with a 12 x 12 window on the GPU: the fused window-12 attention against a chain of CPU oracle operators, the
pool at an even token count against torch, and SwinEngine / the operator chain against the reference's logits."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden, golden_scales

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from test_swin_window12_cpu import tie_block, torch_pool_requant  # noqa: E402

_P = ctypes.c_void_p


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


def P(t):
    return _P(t.data_ptr())


def dyv(d):
    return _lib.Dyadic(float(d[0].m), float(d[0].r))


def chain_window_attention(qkv, relb, dqk, da, dpv, s, R, shift, heads, ws=12):
    """The windowed attention from oracle pieces: roll, partition, q.k^T, qact_attn1, + bias identity (qact2), shift mask,
    8-bit Shiftmax, attn.v, qact3, reverse, roll back.  qkv int8 [B, R, R, 3, heads, 32] -> ctx int8 [B, R*R, heads*32]."""
    B = qkv.shape[0]
    x = np.roll(qkv, (-shift, -shift), axis=(1, 2)) if shift else qkv
    nw = R // ws
    w = x.reshape(B, nw, ws, nw, ws, 3, heads, 32).transpose(0, 1, 3, 2, 4, 5, 6, 7).reshape(B * nw * nw, ws * ws, 3, heads, 32)
    q = w[:, :, 0].transpose(0, 2, 1, 3)
    k = w[:, :, 1].transpose(0, 2, 1, 3)
    v = w[:, :, 2].transpose(0, 2, 1, 3)
    Bw, N = q.shape[0], ws * ws
    S = orc.bmm_nt_i8(q.reshape(-1, N, 32), k.reshape(-1, N, 32))
    a1 = orc.requant(S.reshape(-1, N), dqk, 8)
    ident = np.broadcast_to(relb[None].astype(np.int32), (Bw, heads, N, N)).reshape(-1, N)
    one = orc.dyadic(np.float32(1.0), np.float32(1.0))
    a2 = orc.requant(a1.reshape(-1, N), da, 8, ident, one)
    mask = orc.swin_attn_mask(R, ws, shift) if shift else None
    p = orc.shiftmax_masked(a2.astype(np.int8).reshape(Bw, heads, N, N), s, 8, mask, nw * nw if shift else 1, heads)
    o = orc.bmm_av(p.reshape(-1, N, N), v.reshape(-1, N, 32))
    o = orc.requant(o.reshape(-1, 32), dpv, 8).reshape(Bw, heads, N, 32).transpose(0, 2, 1, 3)
    o = o.reshape(B, nw, nw, ws, ws, heads * 32).transpose(0, 1, 3, 2, 4, 5).reshape(B, R, R, heads * 32)
    if shift:
        o = np.roll(o, (shift, shift), axis=(1, 2))
    return o.reshape(B, R * R, heads * 32).astype(np.int8)


def _peaked_qkv(rng, B, R, heads):
    """random q | k | v with a few large-magnitude rows, so that some Shiftmax rows are peaked and others flat (row sums
    of exp_int beyond 2^24 where order matters)"""
    qkv = rng.integers(-20, 21, (B, R, R, 3, heads, 32)).astype(np.int16)
    big = rng.random((B, R, R)) < 0.15
    qkv[big, 0] = rng.integers(-127, 128, qkv[big, 0].shape)
    qkv[big, 1] = rng.integers(-127, 128, qkv[big, 1].shape)
    qkv[..., 2, :, :] = rng.integers(-128, 128, qkv[..., 2, :, :].shape)
    return np.ascontiguousarray(qkv.astype(np.int8))


@pytest.mark.parametrize("R,shift", [(12, 0), (24, 0), (24, 6), (12, 6)])
@pytest.mark.parametrize("heads", [1, 2, 3, 4])
def test_window12_attention_equals_oracle_chain(H, R, shift, heads):
    rng = np.random.default_rng(1000 * R + 10 * shift + heads)
    B = 2
    qkv = _peaked_qkv(rng, B, R, heads)
    relb = rng.integers(-40, 41, (heads, 144, 144)).astype(np.int16)
    s = np.float32(0.0523)
    dqk = orc.dyadic(np.float32(0.0021), np.float32(0.047))
    da = orc.dyadic(np.float32(0.047), s)
    dpv = orc.dyadic(np.float32(2.0 ** -7 * 0.031), np.float32(0.029))
    ref = chain_window_attention(qkv, relb, dqk, da, dpv, s, R, shift, heads)
    dq, dr = torch.from_numpy(qkv).cuda(), torch.from_numpy(relb).cuda()
    out = torch.full((B, R * R, heads * 32), 77, dtype=torch.int8, device="cuda")
    H.call("ivit_window_attention_fused", P(dq), dyv(dqk), dyv(da), P(dr), float(s), dyv(dpv), P(out), B, R, 12, shift,
           heads, 32)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got, ref), int((got != ref).sum())


@pytest.mark.parametrize("R,shift,cus", [(36, 0, 1), (36, 6, 1), (36, 6, 2), (36, 0, 3), (24, 6, 1)])
def test_window12_attention_many_windows_per_block(R, shift, cus):
    """Blocks that walk several windows (K / V double buffer, its buffer parity, one barrier per window, a partial last
    group): the launcher picks windows per block from the handle's CU share (ivit_set_cu_share), so a small share gives
    8 / 4 / 2 windows per block on a small grid.  B = 3, R = 36: 27 windows, not a multiple of 8, 4 or 2; 2 heads.
    Share 1 CU: ceil(27/8) * 2 = 8 blocks >= 3 * 2 slots -> 8 windows per block; 2 CUs -> 4; 3 CUs -> 2."""
    h = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    h.set_cu_share(cus)
    rng = np.random.default_rng(77 * R + shift + cus)
    B, heads = 3, 2
    qkv = _peaked_qkv(rng, B, R, heads)
    relb = rng.integers(-40, 41, (heads, 144, 144)).astype(np.int16)
    s = np.float32(0.0523)
    dqk = orc.dyadic(np.float32(0.0021), np.float32(0.047))
    da = orc.dyadic(np.float32(0.047), s)
    dpv = orc.dyadic(np.float32(2.0 ** -7 * 0.031), np.float32(0.029))
    ref = chain_window_attention(qkv, relb, dqk, da, dpv, s, R, shift, heads)
    dq, dr = torch.from_numpy(qkv).cuda(), torch.from_numpy(relb).cuda()
    out = torch.full((B, R * R, heads * 32), 77, dtype=torch.int8, device="cuda")
    h.call("ivit_window_attention_fused", P(dq), dyv(dqk), dyv(da), P(dr), float(s), dyv(dpv), P(out), B, R, 12, shift,
           heads, 32)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got, ref), int((got != ref).sum())


def test_window12_attention_row_sum_order(H):
    """Rows whose 8-bit Shiftmax depends on the order of the exp_int row sum (tests/golden/shiftmax144_order_rows.npz):
    with K = 0 the scores are the bias alone, so every query of the window gets one of these rows.  The kernel equals the
    oracle chain (torch's order), and the same chain with a sequential row sum differs — the test pins the order."""
    from shiftmax144 import exps, probs, sum_seq
    g = load_golden("shiftmax144_order_rows.npz")
    rows, s = g["rows"].astype(np.int16), np.float32(g["scale"])
    rng = np.random.default_rng(12)
    B, R, heads = 2, 12, 2
    qkv = np.zeros((B, R, R, 3, heads, 32), np.int8)
    qkv[..., 0, :, :] = rng.integers(-128, 128, qkv[..., 0, :, :].shape)
    qkv[..., 2, :, :] = rng.integers(-128, 128, qkv[..., 2, :, :].shape)
    relb = np.stack([rows[(np.arange(144) + 3 * h) % len(rows)] for h in range(heads)])        # [heads, 144, 144]
    dqk = orc.dyadic(np.float32(0.0021), np.float32(0.047))
    da = orc.dyadic(np.float32(0.047), s)
    dpv = orc.dyadic(np.float32(2.0 ** -7 * 0.031), np.float32(0.029))
    ref = chain_window_attention(qkv, relb, dqk, da, dpv, s, R, 0, heads)
    # the same chain with the sequential row sum
    e = exps(relb.astype(np.int8), s).reshape(-1, 144)
    p_seq = probs(e, sum_seq(e)).reshape(heads, 144, 144)
    v = qkv.reshape(B, R * R, 3, heads, 32)[:, :, 2].transpose(0, 2, 1, 3)                     # one window per image
    o = orc.bmm_av(np.broadcast_to(p_seq[None], (B, heads, 144, 144)).reshape(-1, 144, 144).astype(np.uint16),
                   np.ascontiguousarray(v).reshape(-1, 144, 32))
    alt = orc.requant(o.reshape(-1, 32), dpv, 8).reshape(B, heads, 144, 32).transpose(0, 2, 1, 3).reshape(B, 144, heads * 32)
    assert (alt.astype(np.int8) != ref).any()
    dq, dr = torch.from_numpy(qkv).cuda(), torch.from_numpy(relb).cuda()
    out = torch.full((B, R * R, heads * 32), 77, dtype=torch.int8, device="cuda")
    H.call("ivit_window_attention_fused", P(dq), dyv(dqk), dyv(da), P(dr), float(s), dyv(dpv), P(out), B, R, 12, 0,
           heads, 32)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref)


def test_window12_attention_refusals(H):
    """other windows, R not a multiple of 12 and the table form at window 12 are refused with IvitError"""
    qkv = torch.zeros(1, 24, 24, 3, 1, 32, dtype=torch.int8, device="cuda")
    relb = torch.zeros(1, 144, 144, dtype=torch.int16, device="cuda")
    out = torch.zeros(1, 576, 32, dtype=torch.int8, device="cuda")
    d = _lib.Dyadic(0.5, 1.0)
    for R, win in ((24, 8), (18, 12), (24, 6)):
        with pytest.raises(_lib.IvitError):
            H.call("ivit_window_attention_fused", P(qkv), d, d, P(relb), 0.05, d, P(out), 1, R, win, 0, 1, 32)
    tabs = iv.freeze.shiftmax_tables(np.float32(0.06))
    aq, et, cl = (torch.from_numpy(np.ascontiguousarray(tabs[k])).cuda() for k in ("aq", "t", "cls"))
    with pytest.raises(_lib.IvitError):
        H.call("ivit_window_attention_fused_lut", P(qkv), d, d, P(relb), 0.05, P(aq), P(et), P(cl), int(tabs["NC"]),
               int(tabs["t"].size), int(tabs["dmin"]), d, P(out), 1, 24, 12, 0, 1, 32)


def test_avgpool_even_tokens_equals_torch(H):
    """ivit_avgpool_requant_scaled at L = 144 on a tie-forcing block == torch's adaptive_avg_pool1d then qact3; at L = 49
    it gives exactly what ivit_avgpool_requant gives."""
    s, s_out = np.float32(0.0417), np.float32(0.0213)
    d = orc.dyadic(s, s_out)
    q = tie_block(3, 144, 256, seed=5)
    X = torch.from_numpy(q.astype(np.float32)) * torch.tensor(s)
    pooled = torch.nn.functional.adaptive_avg_pool1d(X.transpose(1, 2), 1).flatten(1)
    z = torch.round(pooled / torch.tensor(s)).numpy().astype(np.float64)
    ref = np.clip(np.rint(z * float(d[0].m) * float(d[0].r)), -128, 127).astype(np.int8)
    assert np.array_equal(ref, torch_pool_requant(q, s, s_out).astype(np.int8))
    dq = torch.from_numpy(q).cuda()
    out = torch.zeros(3, 256, dtype=torch.int8, device="cuda")
    H.call("ivit_avgpool_requant_scaled", P(dq), 3, 144, 256, float(s), dyv(d), P(out))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref)
    with pytest.raises(_lib.IvitError):             # the entry without the scale keeps refusing even token counts
        H.call("ivit_avgpool_requant", P(dq), 3, 144, 256, dyv(d), P(out))
    q49 = np.random.default_rng(2).integers(-128, 128, (3, 49, 256)).astype(np.int8)
    d49 = torch.from_numpy(q49).cuda()
    o1 = torch.zeros(3, 256, dtype=torch.int8, device="cuda")
    o2 = torch.ones(3, 256, dtype=torch.int8, device="cuda")
    H.call("ivit_avgpool_requant", P(d49), 3, 49, 256, dyv(d), P(o1))
    H.call("ivit_avgpool_requant_scaled", P(d49), 3, 49, 256, float(s), dyv(d), P(o2))
    torch.cuda.synchronize()
    assert np.array_equal(o1.cpu().numpy(), o2.cpu().numpy())


def test_swin_engine_micro_window12_golden():
    """SwinEngine(micro_swin_w12): native runner with 1 and 2 slices, the per-operator path and a captured graph's
    replay == the reference's int32 logits"""
    from ivit_amd.swin_engine import SwinEngine
    g = load_golden("micro_swin_w12_b2.npz")
    cfg = iv.SWIN_CONFIGS[str(g["cfg_name"])]
    w = iv.make_swin_weights(cfg, int(g["seed"]))
    eng = SwinEngine(cfg, w, golden_scales(g))
    imgs = torch.from_numpy(iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"]))).cuda()
    assert np.array_equal(eng.forward(imgs).cpu().numpy(), g["logits_int"])
    assert np.array_equal(eng.head_scale, g["logits_scale"])
    assert np.array_equal(eng.forward(imgs, nslices=2).cpu().numpy(), g["logits_int"])
    assert np.array_equal(eng.forward_ops(imgs).cpu().numpy(), g["logits_int"])
    replay = eng.capture(imgs)
    assert np.array_equal(replay().cpu().numpy(), g["logits_int"])
    # exp_tables: the table form exists for window 7 only, so every window-12 layer keeps the arithmetic Shiftmax
    eng_t = SwinEngine(cfg, w, golden_scales(g), exp_tables=True)
    assert not any(k.endswith("attn.exp_aq") for k in eng_t.table)
    assert np.array_equal(eng_t.forward(imgs).cpu().numpy(), g["logits_int"])


def test_swin_base_384_golden():
    """Swin-B at 384 px, window 12: SwinEngine, a 2-slice forward and the operator chain built by the factory ==
    the reference's int32 logits (the chain's pool at L = 144 decides rounding ties as the reference does)"""
    from ivit_amd.swin_engine import SwinEngine
    g = load_golden("swin_base_384_b1.npz")
    cfg = iv.SWIN_CONFIGS[str(g["cfg_name"])]
    w = iv.make_swin_weights(cfg, int(g["seed"]))
    imgs = iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"]))
    eng = SwinEngine(cfg, w, golden_scales(g))
    assert np.array_equal(eng.forward(torch.from_numpy(imgs).cuda()).cpu().numpy(), g["logits_int"])
    two = torch.from_numpy(np.concatenate([imgs, imgs])).cuda()
    assert np.array_equal(eng.forward(two, nslices=2).cpu().numpy(), np.concatenate([g["logits_int"]] * 2))
    del eng
    m = iv.swin_base_patch4_window12_384()
    m.load_float_weights(w).load_act_scales(golden_scales(g))
    iv.freeze_model(m)
    with torch.no_grad():
        acc, scale = m(torch.from_numpy(imgs).cuda())
    assert np.array_equal(acc.cpu().numpy(), g["logits_int"])
    assert np.array_equal(scale.numpy(), g["logits_scale"])


def test_swin_engine_refuses_other_windows():
    from ivit_amd.swin_engine import SwinEngine
    cfg = iv.SwinConfig("w8", img_size=128, num_classes=10, embed_dim=32, depths=(2, 2), num_heads=(1, 2), window_size=8)
    w = iv.make_swin_weights(cfg, 0)
    with pytest.raises(_lib.IvitError):             # refused before anything is frozen or launched
        SwinEngine(cfg, w, {})
