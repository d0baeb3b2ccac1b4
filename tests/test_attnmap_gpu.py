"""Class-token attention maps on the device, bit for bit, no tolerances.  Operator: ivit_attention_cls_probs against the oracle chain
(bmm_nt_i8 row 0 -> requant(dy, 8) -> shiftmax(s, 16)) over the row lengths at which the kernel changes path, with saturating
multipliers, a row of equal scores and the maximum at the last key, p_cls between guard bands; ivit_attention_map_f32 against the
numpy statement in both modes.  Engine: ViTEngine.attention against the REFERENCE's recorded rows (micro fixtures) and the oracle's
capture (DeiT-Tiny), across slice counts, with and without the head, as a replayed graph; and the refusals, which launch nothing."""
import ctypes
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, golden_scales, load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from ivit_amd.predict import attention_map_reference, attention_reference  # noqa: E402

_P = ctypes.c_void_p
GUARD_BYTES = 4096
FILL = 0x5A
HEADS, MEAN = _lib.IVIT_ATTNMAP_HEADS, _lib.IVIT_ATTNMAP_MEAN
INV, UNS, OK = _lib.IVIT_ERR_INVALID, _lib.IVIT_ERR_UNSUPPORTED, _lib.IVIT_OK


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


def P(t, offset=0):
    return _P(t.data_ptr() + offset)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(nbytes):
    """(whole buffer, payload view): `nbytes` of payload between two 4 KiB guards, everything filled with 0x5A"""
    whole = torch.full((GUARD_BYTES + nbytes + GUARD_BYTES,), FILL, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD_BYTES:GUARD_BYTES + nbytes]


def guards_intact(whole, nbytes):
    w = whole.cpu().numpy()
    return bool(np.all(w[:GUARD_BYTES] == FILL) and np.all(w[GUARD_BYTES + nbytes:] == FILL))


def eq16(a, b):
    """torch.equal of two uint16 tensors, through their int16 views"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def err(h):
    return h.lib.ivit_last_error(h.h).decode()


# ---------------------------------------------------------------- 1. the tap kernel alone, against the oracle chain
def oracle_rows(q, k, dy, s):
    """[BH, T] uint16: row 0 of the three-operator chain on the CPU oracle"""
    from oracle import oracle as orc
    sc = orc.bmm_nt_i8(np.ascontiguousarray(q[:, :1]), k)                       # [BH, 1, T] int32
    sc8 = orc.requant(sc, dy, 8)
    return orc.shiftmax(sc8.astype(np.int8), np.float32(s), 16).reshape(q.shape[0], q.shape[1]), sc8.reshape(q.shape[0], -1)


def mk_dy(m, r):
    from oracle import oracle as orc
    dy = (orc.Dyadic * 1)()
    dy[0].m, dy[0].r = float(m), float(r)
    return dy


def run_cls_probs(H, q, k, dy, s):
    BH, T, dh = q.shape
    B, nh = (BH, 1) if BH % 5 else (BH // 5, 5)                                  # B * H = BH either way
    qa, d_q = guarded(q.nbytes)
    ka, d_k = guarded(k.nbytes)
    d_q.copy_(torch.from_numpy(q.reshape(-1).view(np.uint8)))
    d_k.copy_(torch.from_numpy(k.reshape(-1).view(np.uint8)))
    before = (qa.clone(), ka.clone())
    out_all, out = guarded(2 * BH * T)                                           # BH * T odd: the payload ends off a 4-byte boundary
    H.call("ivit_attention_cls_probs", P(d_q), P(d_k), _lib.Dyadic(dy[0].m, dy[0].r), float(s), P(out), B, nh, T, dh)
    torch.cuda.synchronize()
    assert guards_intact(out_all, 2 * BH * T), "wrote outside p_cls"
    assert torch.equal(qa, before[0]) and torch.equal(ka, before[1]), "q or k (or their surroundings) changed"
    return out.cpu().numpy().view(np.uint16).reshape(BH, T)


@pytest.mark.parametrize("BH", [1, 5])                         # 5: the second workgroup has one live wavefront
@pytest.mark.parametrize("dh", [32, 64])
@pytest.mark.parametrize("T", [1, 17, 64, 65, 197, 577])        # one key, a partial wavefront, exactly one key per lane, one more, DeiT, ViT-384
def test_cls_probs_against_the_oracle_chain(H, T, dh, BH):
    rng = np.random.default_rng(1000 * T + 10 * dh + BH)
    s = np.float32(0.0625 + 0.01 * (dh == 64))
    q = rng.integers(-128, 128, size=(BH, T, dh), dtype=np.int64).astype(np.int8)
    k = rng.integers(-128, 128, size=(BH, T, dh), dtype=np.int64).astype(np.int8)
    last = BH - 1
    # the row maximum at key T - 1 (the largest dot product there is for this q row) in the last (image, head)
    k[last, T - 1] = np.where(q[last, 0] >= 0, 127, -128)
    mid = mk_dy(round(2.0 ** 31 / 1.37), 2.0 ** -41)           # |acc| of a random row ~ 5000 sqrt(dh): scores over the int8 range, few clamped
    sat = mk_dy(2.0 ** 31, 1.0)                                 # every non-zero acc saturates the convert and the clamp, at both ends
    neg = mk_dy(-round(2.0 ** 31 / 1.11), 2.0 ** -39)           # a negative multiplier: clamps at both ends, the maximum moves
    for name, dy in (("mid", mid), ("sat", sat), ("neg", neg)):
        want, sc8 = oracle_rows(q, k, dy, s)
        got = run_cls_probs(H, q, k, dy, s)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:4].tolist())
        assert np.array_equal(got, attention_reference(q, k, dy, s)), name
        if name == "sat" and T >= 17:
            assert sc8.min() == -128 and sc8.max() == 127
        if name == "mid":
            assert sc8[last, T - 1] == sc8[last].max() == (127 if T > 1 else sc8[last, 0])
    # a row of equal scores: every key of (image, head) 0 the same vector; and one of all-zero scores
    k2 = k.copy()
    k2[0, :] = k2[0, 0]
    want, sc8 = oracle_rows(q, k2, mid, s)
    assert len(set(sc8[0].tolist())) == 1
    got = run_cls_probs(H, q, k2, mid, s)
    assert np.array_equal(got, want) and len(set(got[0].tolist())) == 1
    k2[0, :] = 0
    assert np.array_equal(run_cls_probs(H, q, k2, sat, s), oracle_rows(q, k2, sat, s)[0])


def test_cls_probs_head_dims_16_and_128(H):
    """the narrowest and the widest head the entry takes"""
    rng = np.random.default_rng(5)
    for dh in (16, 128):
        q = rng.integers(-128, 128, size=(3, 33, dh), dtype=np.int64).astype(np.int8)
        k = rng.integers(-128, 128, size=(3, 33, dh), dtype=np.int64).astype(np.int8)
        dy = mk_dy(round(2.0 ** 31 / 1.9), 2.0 ** -40)
        assert np.array_equal(run_cls_probs(H, q, k, dy, 0.05), oracle_rows(q, k, dy, 0.05)[0]), dh


def test_cls_probs_refusals_write_nothing(H):
    B, nh, T, dh = 2, 3, 17, 32
    n = B * nh * T * dh
    arena = torch.zeros(4 * n + 4096, dtype=torch.int8, device="cuda")        # q, k and room behind them: no refused call could leave it
    q, k = arena[:n], arena[n:2 * n]
    out_all, out = guarded(2 * B * nh * 1100)
    f = H.lib.ivit_attention_cls_probs
    dy = _lib.Dyadic(2.0 ** 20, 2.0 ** -30)
    for args, status, names in (
            ((P(q, 1), P(k), dy, 0.05, P(out), B, nh, T, dh), INV, ("q", "16-byte")),                 # a misaligned q
            ((P(q), P(k, 8), dy, 0.05, P(out), B, nh, T, dh), INV, ("k", "16-byte")),
            ((P(q), P(k), dy, 0.05, P(out, 1), B, nh, T, dh), INV, ("p_cls", "2-byte")),
            ((None, P(k), dy, 0.05, P(out), B, nh, T, dh), INV, ("null",)),
            ((P(q), P(k), dy, 0.05, None, B, nh, T, dh), INV, ("null",)),
            ((P(q), P(k), dy, 0.0, P(out), B, nh, T, dh), INV, ("s_softmax",)),
            ((P(q), P(k), dy, -1.0, P(out), B, nh, T, dh), INV, ("s_softmax",)),
            ((P(q), P(k), dy, float("nan"), P(out), B, nh, T, dh), INV, ("s_softmax",)),
            ((P(q), P(k), dy, float("inf"), P(out), B, nh, T, dh), INV, ("s_softmax",)),
            ((P(q), P(k), dy, 0.05, P(out), 0, nh, T, dh), INV, ("positive",)),
            ((P(q), P(k), dy, 0.05, P(out), B, nh, 0, dh), INV, ("positive",)),
            ((P(q), P(k), dy, 0.05, P(out), B, nh, T, 24), UNS, ("dh",)),                             # not a multiple of 16
            ((P(q), P(k), dy, 0.05, P(out), 1, 1, T, 144), UNS, ("dh",)),                             # beyond 128
            ((P(q), P(k), dy, 0.05, P(out), 1, 1, 1025, 16), UNS, ("T",)),                            # beyond 1024
            # overlap: p_cls inside q, inside k (2-byte aligned is all it needs), the last element of k
            ((P(q), P(k), dy, 0.05, P(q, 2), B, nh, T, dh), INV, ("overlap", "q", "p_cls")),
            ((P(q), P(k), dy, 0.05, P(k), B, nh, T, dh), INV, ("overlap", "k", "p_cls")),
            ((P(q), P(k), dy, 0.05, P(k, n - 2), B, nh, T, dh), INV, ("overlap", "k", "p_cls"))):
        assert f(H.h, *args) == status, (names, err(H))
        for name in names:
            assert name in err(H), (names, err(H))
    assert f(None, P(q), P(k), dy, 0.05, P(out), B, nh, T, dh) == INV
    torch.cuda.synchronize()
    assert bool((out_all == FILL).all()) and int(arena.abs().sum()) == 0, "a refused call wrote"
    # arrays that merely touch are accepted: p_cls directly behind k
    assert f(H.h, P(q), P(k), dy, 0.05, P(arena, 2 * n), B, nh, T, dh) == OK, err(H)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 2. the fp32 map
@pytest.mark.parametrize("T", [2, 17, 197])
@pytest.mark.parametrize("nh", [1, 3, 16])
def test_attention_map_f32_every_bit(H, nh, T):
    rng = np.random.default_rng(100 * nh + T)
    rows = 5
    p = rng.integers(0, 32769, size=(rows, nh, T), dtype=np.int64).astype(np.uint16)
    p[0] = 32768
    p[1] = 0
    p[2, :, 1:] = np.array([0, 1, 32767, 32768], np.uint16)[np.arange(T - 1) % 4]
    p[3] = 1
    pa, d_p = guarded(p.nbytes)
    d_p.copy_(torch.from_numpy(p.reshape(-1).view(np.uint8)))
    before = pa.clone()
    for mode, heads in ((HEADS, True), (MEAN, False)):
        want = attention_map_reference(p, heads=heads)
        out_all, out = guarded(want.nbytes)
        H.call("ivit_attention_map_f32", P(d_p), rows, nh, T, mode, P(out))
        torch.cuda.synchronize()
        assert guards_intact(out_all, want.nbytes), "wrote outside its output"
        got = out.cpu().numpy().view(np.float32).reshape(want.shape)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (mode, np.argwhere(got != want)[:4].tolist())
    assert torch.equal(pa, before), "p_cls or its surroundings changed"


def test_attention_map_f32_refusals_and_empty_calls(H):
    p = torch.zeros(4 * 600 * 20, dtype=torch.int16, device="cuda")
    out_all, out = guarded(4 * 4 * 600 * 20)
    f = H.lib.ivit_attention_map_f32
    for args, status, names in (
            ((P(p), 4, 3, 17, 2, P(out)), INV, ("mode",)),
            ((P(p), 4, 3, 17, -1, P(out)), INV, ("mode",)),
            ((None, 4, 3, 17, MEAN, P(out)), INV, ("p_cls",)),
            ((P(p), 4, 3, 17, MEAN, None), INV, ("out",)),
            ((P(p), -1, 3, 17, MEAN, P(out)), INV, ("rows",)),
            ((P(p), 4, 0, 17, MEAN, P(out)), INV, ("H",)),
            ((P(p), 4, 3, 0, MEAN, P(out)), INV, ("T",)),
            ((P(p, 1), 4, 3, 17, MEAN, P(out)), INV, ("p_cls", "2-byte")),
            ((P(p), 4, 3, 17, MEAN, P(out, 2)), INV, ("out", "4-byte")),
            ((P(p), 4, 3, 17, HEADS, P(p, 4)), INV, ("overlap", "p_cls", "out")),
            ((P(p), 4, 3, 17, MEAN, P(p, 4 * 3 * 17 * 2 - 4)), INV, ("overlap", "p_cls", "out")),
            ((P(p), 4, 512, 17, MEAN, P(out)), UNS, ("H",)),
            ((P(p), 4, 3, 1025, HEADS, P(out)), UNS, ("T",))):
        assert f(H.h, *args) == status, (names, err(H))
        for name in names:
            assert name in err(H), (names, err(H))
    assert f(H.h, P(p), 0, 3, 17, MEAN, P(out)) == OK and f(H.h, P(p), 4, 3, 1, HEADS, P(out)) == OK      # nothing to do: nothing launched
    torch.cuda.synchronize()
    assert bool((out_all == FILL).all()) and int(p.abs().sum()) == 0, "a refused or empty call wrote"


# ---------------------------------------------------------------- 3. the engine against the reference's rows
def _vit(fname):
    from ivit_amd.engine import ViTEngine
    from oracle import oracle as orc
    g = load_golden(fname)
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    w = iv.make_vit_weights(cfg, int(g["seed"]))
    return g, cfg, ViTEngine.from_float(cfg, w, golden_scales(g)), orc.OracleViT(cfg, w, golden_scales(g))


def _check_maps(attn16, maps, heads, cfg):
    """maps are the numpy statement of attn16, on the patch grid"""
    a = attn16.cpu().numpy()
    grid = cfg.img_size // cfg.patch_size
    want = attention_map_reference(a, heads=heads)
    assert maps.dtype == torch.float32 and maps.shape == want.shape[:-1] + (grid, grid)
    assert np.array_equal(maps.cpu().numpy().reshape(want.shape).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("fname", ["micro_vit_b2.npz", "micro_vit2h_b3.npz"])
def test_engine_attention_equals_the_recorded_rows(fname):
    g, cfg, eng, _ = _vit(fname)
    imgs = dev(iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"])))
    B, nh, T = imgs.shape[0], cfg.num_heads, cfg.num_tokens
    attn16, maps, logits = eng.attention(imgs, blocks=(0, 1), logits=True)
    assert attn16.dtype == torch.uint16 and attn16.shape == (2, B, nh, T)
    for t, i in enumerate((0, 1)):
        want = g[f"site/blocks.{i}.attn.int_softmax"][:, :, 0, :]
        assert np.array_equal(attn16[t].cpu().numpy(), want), (fname, i)
    assert np.array_equal(logits.cpu().numpy(), g["logits_int"]) and logits.data_ptr() == eng.last_logits.data_ptr()
    _check_maps(attn16, maps, False, cfg)
    a2, m2 = eng.attention(imgs, blocks=-1, heads=True)                     # the default: the last block
    assert a2.shape == (1, B, nh, T) and np.array_equal(a2[0].cpu().numpy(), g["site/blocks.1.attn.int_softmax"][:, :, 0, :])
    _check_maps(a2, m2, True, cfg)
    # every row is a distribution to within the floor chain: at most T counts below 2^15
    tot = a2.cpu().numpy().astype(np.int64).sum(axis=-1)
    assert np.all((tot <= 32768) & (tot > 32768 - 2 * T))


def test_engine_attention_deit_tiny_equals_the_oracle_capture():
    g, cfg, eng, o = _vit("deit_tiny_b1.npz")
    host = iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"]))
    cap = {}
    ref_logits, _ = o.forward(host, capture=cap)
    blocks = (0, 5, 11)
    attn16, maps, logits = eng.attention(dev(host), blocks=blocks, logits=True)
    assert attn16.shape == (3, host.shape[0], 3, 197) and maps.shape == (3, host.shape[0], 14, 14)
    for t, i in enumerate(blocks):
        assert np.array_equal(attn16[t].cpu().numpy(), cap[f"blocks.{i}.attn.int_softmax"][:, :, 0, :]), i
    assert np.array_equal(logits.cpu().numpy(), ref_logits) and np.array_equal(ref_logits, g["logits_int"])
    _check_maps(attn16, maps, False, cfg)
    headless = eng.attention(dev(host), blocks=(-12, -7, -1), copy=True)     # the same blocks from the end, no head
    assert len(headless) == 2 and eq16(headless[0], attn16)


def test_engine_attention_on_the_three_launch_chain_head_dim_32():
    """a model outside the fused attention (head dim 32: qk -> Shiftmax -> pv as three launches on whole matrices): the tap sits behind
    its qkv launch just the same, ragged slices included"""
    from oracle import oracle as orc
    cfg = iv.ViTConfig("attnmap32", img_size=24, patch_size=8, num_classes=7, embed_dim=64, depth=2, num_heads=2)
    assert cfg.head_dim == 32
    w = iv.make_vit_weights(cfg, seed=5)
    m = iv.VisionTransformer(img_size=24, patch_size=8, num_classes=7, embed_dim=64, depth=2, num_heads=2, mlp_ratio=4)
    m.load_float_weights(w)
    with torch.no_grad():
        m(dev(iv.make_calibration_batch(cfg, 3, seed=17)))
    iv.freeze_model(m)
    sc = {k: v for k, v in m.act_scales().items() if v > 0}
    eng = m.compile()
    assert not eng.fused_attention
    imgs = iv.make_images_int8(cfg, 5, seed=23)
    cap = {}
    ref, _ = orc.OracleViT(cfg, w, sc).forward(imgs, capture=cap)
    want = np.stack([cap[f"blocks.{i}.attn.int_softmax"][:, :, 0, :] for i in range(2)])
    for ns in (3, 1):
        attn16, maps, logits = eng.attention(dev(imgs), blocks=(0, 1), logits=True, nslices=ns)
        assert np.array_equal(attn16.cpu().numpy(), want) and np.array_equal(logits.cpu().numpy(), ref), ns
        _check_maps(attn16, maps, False, cfg)
        assert np.array_equal(eng.attention(dev(imgs), blocks=0, nslices=ns)[0].cpu().numpy(), want[:1]), ns


# ---------------------------------------------------------------- 4 - 6. slices, the head, the logits buffer, the graph
B5 = 5


@pytest.fixture(scope="module")
def model():
    g, cfg, eng, o = _vit("micro_vit2h_b3.npz")
    host = iv.make_images_int8(cfg, B5, seed=53)
    cap = {}
    ref_logits, _ = o.forward(host, capture=cap)
    rows = np.stack([cap[f"blocks.{i}.attn.int_softmax"][:, :, 0, :] for i in range(cfg.depth)])       # [depth, B, H, T], computed once
    rows.setflags(write=False)
    return g, cfg, eng, o, dev(host), rows, ref_logits


def test_attention_across_slices_with_and_without_the_head(model):
    g, cfg, eng, o, imgs, rows, ref_logits = model
    fwd = eng.forward(imgs, copy=True)
    assert np.array_equal(fwd.cpu().numpy(), ref_logits)
    for nslices in (1, 2, 3):                                                    # 5 images: slices of 5; 2 + 3; 1 + 2 + 2
        for blocks in ((0, 1), (0,), (1,)):
            want = rows[list(blocks)]
            # 5. without the head the logits buffer of this shape keeps whatever it held
            lg = eng.forward(imgs, nslices=nslices)
            lg.fill_(0x5A5A5A5A)
            attn16, maps = eng.attention(imgs, blocks=blocks, nslices=nslices)
            assert np.array_equal(attn16.cpu().numpy(), want), (nslices, blocks)
            assert bool((eng._native_buffers(B5, nslices)[1] == 0x5A5A5A5A).all()), (nslices, blocks)
            _check_maps(attn16, maps, False, cfg)
            a2, m2, logits = eng.attention(imgs, blocks=blocks, heads=True, logits=True, nslices=nslices, copy=True)
            assert np.array_equal(a2.cpu().numpy(), want) and torch.equal(logits, fwd), (nslices, blocks)
            _check_maps(a2, m2, True, cfg)
    # forward is what it was after all of that
    assert torch.equal(eng.forward(imgs), fwd)
    # the engine's own buffers, and copies
    a = eng.attention(imgs)
    b = eng.attention(imgs, copy=True)
    assert a[0].data_ptr() == eng.attention(imgs)[0].data_ptr() != b[0].data_ptr() and eq16(a[0], b[0]) and torch.equal(a[1], b[1])
    for bad in ((1, 0), (0, 0), (2,), (), (0, -2), 2, -3):
        with pytest.raises(ValueError):
            eng.attention(imgs, blocks=bad)


def test_headless_attention_writes_no_logits_through_the_c_entry(model):
    """the C entry on the test's own buffers: logits NULL, a guard-banded logits-sized buffer beside attn16 stays untouched, and so do
    the bands around attn16 and map32 (odd T: the planes' ends lie off 4-byte boundaries)"""
    g, cfg, eng, o, imgs, rows, _ = model
    nh, T = cfg.num_heads, cfg.num_tokens
    ws, _ = eng._native_buffers(B5, 2)
    lg_all, lg = guarded(4 * B5 * cfg.num_classes)
    a_all, a16 = guarded(2 * 1 * B5 * nh * T)
    m_all, m32 = guarded(4 * 1 * B5 * (T - 1))
    blocks = (ctypes.c_int * 1)(1)
    eng._use_current_stream()
    st = eng.h.lib.ivit_vit_attention(eng.model, P(imgs), B5, 2, P(ws), ws.numel(), None, blocks, 1, P(a16), MEAN, P(m32))
    assert st == OK, err(eng.h)
    torch.cuda.synchronize()
    assert bool((lg_all == FILL).all()), "logits written without a logits argument"
    assert guards_intact(a_all, a16.numel()) and guards_intact(m_all, m32.numel())
    got = a16.cpu().numpy().view(np.uint16).reshape(1, B5, nh, T)
    assert np.array_equal(got, rows[[1]])
    want = attention_map_reference(got, heads=False)
    assert np.array_equal(m32.cpu().numpy().view(np.uint32).reshape(want.shape), want.view(np.uint32))
    # map32 NULL: attn16 alone; with logits, one slice
    a16.fill_(FILL)
    ws, _ = eng._native_buffers(B5, 1)
    st = eng.h.lib.ivit_vit_attention(eng.model, P(imgs), B5, 1, P(ws), ws.numel(), P(lg), blocks, 1, P(a16), HEADS, None)
    assert st == OK, err(eng.h)
    torch.cuda.synchronize()
    assert np.array_equal(a16.cpu().numpy().view(np.uint16).reshape(1, B5, nh, T), rows[[1]])
    assert torch.equal(lg.view(torch.int32).view(B5, -1), eng.forward(imgs)) and guards_intact(lg_all, lg.numel())


def test_capture_attention_replays_on_refilled_images(model):
    g, cfg, eng, _, _, _, _ = model
    B = 3
    buf = dev(iv.make_images_int8(cfg, B, seed=1))
    replay = eng.capture_attention(buf, blocks=(0, 1), logits=True, nstreams=2)
    buf1 = buf.clone()
    headless = eng.capture_attention(buf1, blocks=-1, heads=True, nstreams=1)
    for seed in (61, 62):
        imgs = dev(iv.make_images_int8(cfg, B, seed=seed))
        want16, want32, want_logits = eng.attention(imgs, blocks=(0, 1), logits=True, copy=True)
        last16, last32 = eng.attention(imgs, blocks=(1,), heads=True, copy=True)
        assert eq16(last16[0], want16[1])
        buf.copy_(imgs)
        a16, m32, logits = replay()
        torch.cuda.synchronize()
        assert eq16(a16, want16) and torch.equal(m32.view(torch.int32), want32.view(torch.int32)) and torch.equal(logits, want_logits), seed
        buf1.copy_(imgs)
        h16, h32 = headless()
        torch.cuda.synchronize()
        assert eq16(h16, last16) and torch.equal(h32.view(torch.int32), last32.view(torch.int32)), seed


# ---------------------------------------------------------------- 7. the runner's refusals
def test_vit_attention_refusals_launch_nothing(model):
    g, cfg, eng, _, imgs, _, _ = model
    nh, T, B = cfg.num_heads, cfg.num_tokens, B5
    ws, _ = eng._native_buffers(B, 1)
    # one size for all five arrays, the largest extent among them: even a call that were NOT refused would stay inside them
    sizes = {"images": imgs.numel(), "workspace": ws.numel(), "logits": 4 * B * cfg.num_classes, "attn16": 2 * 2 * B * nh * T,
             "map32": 4 * 2 * B * nh * (T - 1)}
    big = max(sizes.values()) + 256
    arena = {n: torch.full((big,), FILL, dtype=torch.uint8, device="cuda") for n in sizes}
    arena["images"][:imgs.numel()].copy_(imgs.reshape(-1).view(torch.uint8))
    assert all(a.data_ptr() % 256 == 0 for a in arena.values())
    f = eng.h.lib.ivit_vit_attention
    eng._use_current_stream()

    def call(blocks=(0, 1), mode=HEADS, **ptr):
        p = {n: P(arena[n]) for n in sizes}
        p.update(ptr)
        arr = (ctypes.c_int * max(len(blocks), 1))(*blocks) if blocks is not None else None
        return f(eng.model, p["images"], B, 1, p["workspace"], big, p["logits"], arr, len(blocks) if blocks is not None else 1,
                 p["attn16"], mode, p["map32"])
    for blocks in ((1, 0), (0, 0), (0, 2), (-1,), (2,), (), (0, 1, 1), None):                 # depth = 2
        assert call(blocks=blocks) == INV and "blocks_host" in err(eng.h), (blocks, err(eng.h))
    assert call(attn16=None) == INV and "attn16" in err(eng.h)
    for mode in (2, -1):
        assert call(mode=mode) == INV and "mode" in err(eng.h)
        assert call(mode=mode, map32=None) == INV and "mode" in err(eng.h)                    # judged without a map too
    assert call(attn16=P(arena["attn16"], 1)) == INV and "attn16" in err(eng.h) and "2-byte" in err(eng.h)
    assert call(map32=P(arena["map32"], 2)) == INV and "map32" in err(eng.h) and "4-byte" in err(eng.h)
    assert call(workspace=P(arena["workspace"], 16)) == INV and "workspace" in err(eng.h)
    # each overlapping pair: the second array put on the first one's start, and on its last bytes
    names = list(sizes)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            for at in (0, (sizes[a] - 4) // 256 * 256):
                assert call(**{b: P(arena[a], at)}) == INV, (a, b, at)
                e = err(eng.h)
                assert "overlap" in e and a in e and b in e and "ivit_vit_attention" in e, (a, b, e)
    torch.cuda.synchronize()
    for n, a in arena.items():
        if n == "images":
            assert torch.equal(a[:imgs.numel()], imgs.reshape(-1).view(torch.uint8)) and bool((a[imgs.numel():] == FILL).all())
        else:
            assert bool((a == FILL).all()), f"a refused call wrote {n}"
    # the same arguments, nothing wrong with them: accepted (the refusals above were about what they said)
    eng._workspace_init(arena["workspace"], B, 1)
    assert call() == OK, err(eng.h)
    torch.cuda.synchronize()
    got = arena["attn16"][:sizes["attn16"]].cpu().numpy().view(np.uint16).reshape(2, B, nh, T)
    assert np.array_equal(got, model[5])
    assert np.array_equal(arena["logits"][:sizes["logits"]].cpu().numpy().view(np.int32).reshape(B, -1), model[6])


# ---------------------------------------------------------------- the tool
def test_attention_map_tool_writes_what_the_engine_returns(model, tmp_path, capsys, monkeypatch):
    """tools/attention_map.py, in this process, on a small file of int8 model inputs"""
    g, cfg, eng, _, _, _, _ = model
    images = iv.make_images_int8(cfg, 5, seed=81)
    labels = np.arange(5, dtype=np.int64) % cfg.num_classes
    data, out = str(tmp_path / "data.npz"), str(tmp_path / "maps.npz")
    np.savez(data, images=images, labels=labels)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))
    spec = importlib.util.spec_from_file_location("ivit_tools_attention_map", os.path.join(ROOT, "tools", "attention_map.py"))
    tool = importlib.util.module_from_spec(spec)
    try:
        spec.loader.exec_module(tool)
    finally:
        sys.modules.pop("evaluate", None)                                        # tools/evaluate.py, which the tool shares its loading with
    base = ["attention_map.py", data, "--model", str(g["cfg_name"]), "--golden", os.path.join(ROOT, "tests", "golden", "micro_vit2h_b3.npz"),
            "--out", out, "--batch", "2"]
    for extra, blocks, heads in ((["--blocks", "0", "-1", "--topk", "3"], (0, 1), False), (["--heads"], (1,), True)):
        monkeypatch.setattr(sys, "argv", base + extra)
        tool.main()
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert line["n"] == 5 and line["blocks"] == list(blocks) and line["heads"] is heads and line["grid"] == [4, 4]
        z = np.load(out)
        want16, want32, logits = eng.attention(dev(images), blocks=blocks, heads=heads, logits=True, copy=True)
        assert z["attn16"].dtype == np.uint16 and np.array_equal(z["attn16"], want16.cpu().numpy())
        assert np.array_equal(z["maps"].view(np.uint32), want32.cpu().numpy().view(np.uint32)) and z["maps"].shape == tuple(want32.shape)
        assert np.array_equal(z["labels"], labels) and np.array_equal(z["blocks"], blocks)
        if "--topk" in extra:
            from ivit_amd.predict import topk_reference
            idx, val = topk_reference(logits.cpu().numpy(), eng.head_scale_host(), 3)
            assert np.array_equal(z["topk_idx"], idx) and np.array_equal(z["topk_val"].view(np.uint32), val.view(np.uint32))
        else:
            assert "topk_idx" not in z.files
    monkeypatch.setattr(sys, "argv", base + ["--blocks", "1", "0"])
    with pytest.raises(ValueError):
        tool.main()
