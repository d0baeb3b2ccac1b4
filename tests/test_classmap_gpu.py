"""Class-activation maps of a Swin on the device, every integer and every fp32 bit, no tolerances.  Operator: ivit_class_map against
`class_map_reference` over the token counts at which a lane owns 0, 1, 2 or 3 tokens, the narrowest and the widest row, and class
slots that do not fill a block's four wavefronts, between guard bands, with and without map32; the extreme sum; indices out of
range; its refusals.  Engine: SwinEngine.class_map against the REFERENCE's recorded tokens (site/qact2, csum/qact2), across slice
counts and both modes, with and without the head, as a replayed graph; the runner's refusals, which launch nothing; the tool."""
import ctypes
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, csum, load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from ivit_amd.predict import class_map_reference, topk_reference  # noqa: E402
from test_predict_gpu import H, _engine, dev  # noqa: E402,F401  (H: the module's handle fixture)

_P = ctypes.c_void_p
GUARD_BYTES = 4096
FILL = 0x5A
TOPK, GIVEN = _lib.IVIT_CLASSMAP_TOPK, _lib.IVIT_CLASSMAP_GIVEN
INV, UNS, OK = _lib.IVIT_ERR_INVALID, _lib.IVIT_ERR_UNSUPPORTED, _lib.IVIT_OK


def P(t, offset=0):
    return _P(t.data_ptr() + offset)


def guarded(nbytes):
    """(whole buffer, payload view): `nbytes` of payload between two 4 KiB guards, everything filled with 0x5A"""
    whole = torch.full((GUARD_BYTES + nbytes + GUARD_BYTES,), FILL, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD_BYTES:GUARD_BYTES + nbytes]


def guards_intact(whole, nbytes):
    w = whole.cpu().numpy()
    return bool(np.all(w[:GUARD_BYTES] == FILL) and np.all(w[GUARD_BYTES + nbytes:] == FILL))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def err(h):
    return h.lib.ivit_last_error(h.h).decode()


# ---------------------------------------------------------------- 1. the operator alone
def run_class_map(H, tok8, head_w, idx, class_scale):
    """ivit_class_map on host arrays -> (cam32, map32 or None); the guards around both outputs and the bytes of tok8 and idx (and
    around them) must stay what they were"""
    B, L, C = tok8.shape
    ncls, k = head_w.shape[0], idx.shape[1]
    t_all, d_tok = guarded(tok8.nbytes)
    i_all, d_idx = guarded(idx.nbytes)
    d_tok.copy_(torch.from_numpy(tok8.reshape(-1).view(np.uint8)))
    d_idx.copy_(torch.from_numpy(idx.reshape(-1).view(np.uint8)))
    before = (t_all.clone(), i_all.clone())
    d_w, d_s = dev(head_w), dev(class_scale) if class_scale is not None else None
    n = 4 * B * k * L
    c_all, cam = guarded(n)
    m_all, m32 = guarded(n)
    H.call("ivit_class_map", P(d_tok), P(d_w), P(d_idx), B, L, C, ncls, k, P(d_s) if d_s is not None else None, P(cam),
           P(m32) if d_s is not None else None)
    torch.cuda.synchronize()
    assert guards_intact(c_all, n) and guards_intact(m_all, n), "wrote outside its outputs"
    assert torch.equal(t_all, before[0]) and torch.equal(i_all, before[1]), "tok8 or idx (or their surroundings) changed"
    if d_s is None:
        assert bool((m32 == FILL).all()), "map32 written without being asked for"
    return cam.cpu().numpy().view(np.int32).reshape(B, k, L), m32.cpu().numpy().view(np.float32).reshape(B, k, L) if d_s is not None else None


def check_class_map(H, tok8, head_w, idx, class_scale):
    want_cam, want_map = class_map_reference(tok8, head_w, idx, class_scale)
    cam, m32 = run_class_map(H, tok8, head_w, idx, class_scale)
    assert np.array_equal(cam, want_cam), np.argwhere(cam != want_cam)[:4].tolist()
    assert np.array_equal(bits(m32), bits(want_map)), np.argwhere(bits(m32) != bits(want_map))[:4].tolist()
    cam_only, none = run_class_map(H, tok8, head_w, idx, None)                     # the other instantiation
    assert none is None and np.array_equal(cam_only, want_cam)


NCLS = 37


@pytest.mark.parametrize("C", [16, 64, 1024])                   # one 16-byte piece, the micro model's row, the widest row there is
@pytest.mark.parametrize("L", [1, 49, 64, 65, 144])             # lanes with 0 and 1 token; 0 / 1; exactly 1; 1 / 2; 2 / 3
def test_class_map_every_integer_and_bit(H, L, C):
    rng = np.random.default_rng(1000 * L + C)
    head_w = rng.integers(-127, 128, size=(NCLS, C), dtype=np.int64).astype(np.int8)
    class_scale = rng.uniform(1e-6, 1e-3, size=NCLS).astype(np.float32)
    class_scale[rng.random(NCLS) < 0.3] *= -1
    for batch in (1, 3, 5):                                     # with k = 1 and 5: B * k = 1, 3, 5, 15, 25 — no multiple of a block's four waves
        tok8 = rng.integers(-128, 128, size=(batch, L, C), dtype=np.int64).astype(np.int8)
        for k in (1, 5, 16):
            idx = rng.integers(0, NCLS, size=(batch, k), dtype=np.int64).astype(np.int32)
            check_class_map(H, tok8, head_w, idx, class_scale)


def test_class_map_extreme_sum_stays_exact(H):
    """tok8 all -128 against a weight row all -127 at C = 1024: 16 646 144 < 2^24, exact in int32 and in fp32; and the opposite sign"""
    tok8 = np.full((2, 65, 1024), -128, np.int8)
    head_w = np.full((3, 1024), -127, np.int8)
    head_w[1] = 127
    idx = np.array([[0, 1, 2], [1, 1, 0]], np.int32)
    scale = np.array([1.0, 0.75, 2.0 ** -20], np.float32)
    cam, m32 = run_class_map(H, tok8, head_w, idx, scale)
    assert np.all(cam[0, 0] == 16646144) and np.all(cam[0, 1] == -16646144) and np.all(m32[0, 0] == np.float32(16646144.0))
    check_class_map(H, tok8, head_w, idx, scale)


def test_class_map_indices_out_of_range_and_duplicates(H):
    rng = np.random.default_rng(5)
    tok8 = rng.integers(-128, 128, size=(3, 49, 64), dtype=np.int64).astype(np.int8)
    head_w = rng.integers(-127, 128, size=(10, 64), dtype=np.int64).astype(np.int8)
    scale = rng.uniform(1e-4, 1e-3, size=10).astype(np.float32)
    idx = np.array([[4, 4, -1, 10, 9], [-2 ** 31, 2 ** 31 - 1, 0, 0, 10], [9, 8, 7, 6, 5]], np.int32)
    cam, m32 = run_class_map(H, tok8, head_w, idx, scale)
    for b, j in ((0, 2), (0, 3), (1, 0), (1, 1), (1, 4)):
        assert not cam[b, j].any() and np.all(bits(m32[b, j]) == 0x7FC00000), (b, j)
    assert np.array_equal(cam[0, 0], cam[0, 1]) and cam[0, 0].any() and np.array_equal(bits(m32[1, 2]), bits(m32[1, 3]))
    check_class_map(H, tok8, head_w, idx, scale)


def test_class_map_refusals_write_nothing(H):
    B, L, C, k, ncls = 3, 49, 64, 5, 10
    big = torch.zeros(B * L * 1040 + 64, dtype=torch.int8, device="cuda")          # tok8 and head_w for every width tried
    d_idx = torch.zeros(B, 17, dtype=torch.int32, device="cuda")
    d_s = torch.ones(ncls, dtype=torch.float32, device="cuda")
    n = 4 * B * 17 * L
    c_all, cam = guarded(n)
    m_all, m32 = guarded(n)
    f = H.lib.ivit_class_map
    ok = dict(tok8=P(big), head_w=P(big), idx=P(d_idx), batch=B, L=L, C=C, ncls=ncls, k=k, scale=P(d_s), cam32=P(cam), map32=P(m32))

    def call(**kw):
        a = dict(ok, **kw)
        return f(H.h, a["tok8"], a["head_w"], a["idx"], a["batch"], a["L"], a["C"], a["ncls"], a["k"], a["scale"], a["cam32"], a["map32"])
    nidx, nmap = 4 * B * k, 4 * B * k * L
    for kw, status, names in (
            (dict(C=24), UNS, ("C",)), (dict(C=1040), UNS, ("C",)),                                   # not a multiple of 16; beyond 1024
            (dict(k=17), INV, ("k",)), (dict(k=0), INV, ("k",)),
            (dict(batch=0), INV, ("batch",)), (dict(L=0), INV, ("L",)), (dict(ncls=0), INV, ("num_classes",)),
            (dict(tok8=P(big, 8)), INV, ("tok8", "16-byte")), (dict(head_w=P(big, 4)), INV, ("head_w", "16-byte")),
            (dict(cam32=P(cam, 2)), INV, ("cam32", "4-byte")), (dict(map32=P(m32, 2)), INV, ("map32", "4-byte")),
            (dict(idx=P(d_idx, 2)), INV, ("idx", "4-byte")),
            (dict(map32=None), INV, ("class_scale", "map32")), (dict(scale=None), INV, ("class_scale", "map32")),
            (dict(tok8=None), INV, ("tok8",)), (dict(head_w=None), INV, ("head_w",)), (dict(idx=None), INV, ("idx",)),
            (dict(cam32=None, map32=None, scale=None), INV, ("cam32",)),
            # each overlapping pair: the output on the other array's start, and on its last bytes
            (dict(cam32=P(big)), INV, ("overlap", "tok8", "cam32")), (dict(cam32=P(big, B * L * C - 4)), INV, ("overlap", "tok8", "cam32")),
            (dict(map32=P(big)), INV, ("overlap", "tok8", "map32")), (dict(map32=P(big, B * L * C - 4)), INV, ("overlap", "tok8", "map32")),
            (dict(cam32=P(d_idx)), INV, ("overlap", "idx", "cam32")), (dict(cam32=P(d_idx, nidx - 4)), INV, ("overlap", "idx", "cam32")),
            (dict(map32=P(d_idx)), INV, ("overlap", "idx", "map32")), (dict(map32=P(d_idx, nidx - 4)), INV, ("overlap", "idx", "map32")),
            (dict(map32=P(cam)), INV, ("overlap", "cam32", "map32")), (dict(map32=P(cam, nmap - 4)), INV, ("overlap", "cam32", "map32")),
            (dict(cam32=P(m32, nmap - 4)), INV, ("overlap", "cam32", "map32"))):
        assert call(**kw) == status, (kw.keys(), err(H))
        for name in names:
            assert name in err(H), (names, err(H))
    assert f(None, *[ok[n_] for n_ in ("tok8", "head_w", "idx", "batch", "L", "C", "ncls", "k", "scale", "cam32", "map32")]) == INV
    torch.cuda.synchronize()
    assert bool((c_all == FILL).all()) and bool((m_all == FILL).all()), "a refused call wrote"
    assert int(big.abs().sum()) == 0 and int(d_idx.abs().sum()) == 0
    assert call() == OK, err(H)                                                                   # nothing wrong with the rest
    torch.cuda.synchronize()
    assert guards_intact(c_all, nmap) and not cam[:nmap].any()                                    # zeros against zeros


# ---------------------------------------------------------------- 2. the engine against the reference's recordings
def head_integers(eng):
    o, _, shp = eng.table["head.w"]
    return eng.blob[o:o + int(np.prod(shp))].cpu().numpy().view(np.int8).reshape(shp)


def check_outputs(eng, cfg, out, k, B):
    """shapes and types of class_map's results, and cam32 / maps as the numpy statement of the engine's own tok8 and idx"""
    idx, val, tok8, cam32, maps = out
    g = cfg.grid >> (cfg.num_layers - 1)
    assert tok8.dtype == torch.int8 and tok8.shape == (B, g * g, eng.num_features)
    assert idx.dtype == torch.int32 and idx.shape == (B, k) and cam32.dtype == torch.int32 and cam32.shape == (B, k, g * g)
    assert maps.dtype == torch.float32 and maps.shape == (B, k, g, g)
    want_cam, want_map = class_map_reference(tok8.cpu().numpy(), head_integers(eng), idx.cpu().numpy(), eng.class_scale.cpu().numpy())
    assert np.array_equal(cam32.cpu().numpy(), want_cam)
    assert np.array_equal(bits(maps.cpu().numpy().reshape(want_map.shape)), bits(want_map))


def test_engine_class_map_equals_the_recorded_tokens_micro_swin():
    g, cfg, eng = _engine("micro_swin_b2.npz")
    sd = load_golden("micro_swin_state_dict.npz")
    imgs = dev(iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"])))
    B, ncls = imgs.shape[0], cfg.num_classes
    head_w = sd["buf/head.weight_integer"].astype(np.int8)
    assert np.array_equal(head_integers(eng), head_w)
    # the unit of a map: qact2's scale times the head's weight scale, one float32 multiply, outside the constants blob
    assert np.float32(eng.token_scale_host()) == g["scale/qact2"]
    want_scale = (np.float32(g["scale/qact2"]) * sd["buf/head.fc_scaling_factor"]).astype(np.float32)
    assert eng.class_scale.dtype == torch.float32 and np.array_equal(bits(eng.class_scale.cpu().numpy()), bits(want_scale))
    fwd = eng.forward(imgs, copy=True)
    assert np.array_equal(fwd.cpu().numpy(), g["logits_int"])
    for k in (1, 5, 10):
        eng.forward(imgs).zero_()                                                # class_map must write the logits buffer itself
        out = idx, val, tok8, cam32, maps = eng.class_map(imgs, k=k)
        site = g["site/qact2"]
        assert site.shape == tuple(tok8.shape) == (B, 49, 64) and np.array_equal(tok8.cpu().numpy().astype(np.int64), site.astype(np.int64))
        ri, rv = topk_reference(g["logits_int"], g["logits_scale"], k)
        assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(bits(val.cpu().numpy()), bits(rv))
        assert np.array_equal(cam32.cpu().numpy(), class_map_reference(site.astype(np.int8), head_w, ri)[0])
        assert torch.equal(eng.last_logits, fwd) and eng.last_logits.data_ptr() == eng._native_buffers(B, 1)[1].data_ptr()
        check_outputs(eng, cfg, out, k, B)
    for bad_k in (0, 17, 11):                                                    # 11 classes of 10: the top-k has no such k
        with pytest.raises(_lib.IvitError):
            eng.class_map(imgs, k=bad_k)
    with pytest.raises(ValueError):
        eng.class_map(imgs, logits=False)


@pytest.mark.parametrize("fname,L,C", [("micro_swin_w12_b2.npz", 144, 64), ("swin_tiny_b1.npz", 49, 768)])
def test_engine_class_map_equals_the_recorded_checksum(fname, L, C):
    """the even-count pool (L = 144) and the full width of Swin-T: the tokens through their recorded checksum"""
    g, cfg, eng = _engine(fname)
    imgs = dev(iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"])))
    out = idx, val, tok8, cam32, maps = eng.class_map(imgs, k=5)
    assert tuple(tok8.shape) == (imgs.shape[0], L, C) and np.float32(eng.token_scale_host()) == g["scale/qact2"]
    assert csum(tok8.cpu().numpy()) == g["csum/qact2"]
    assert np.array_equal(eng.last_logits.cpu().numpy(), g["logits_int"])
    ri, rv = topk_reference(g["logits_int"], g["logits_scale"], 5)
    assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(bits(val.cpu().numpy()), bits(rv))
    check_outputs(eng, cfg, out, 5, imgs.shape[0])


# ---------------------------------------------------------------- 3. slices, modes, the head, the graph
B5 = 5


@pytest.fixture(scope="module")
def model():
    g, cfg, eng = _engine("micro_swin_b2.npz")
    imgs = dev(iv.make_images_int8(cfg, B5, seed=53))
    fwd = eng.forward(imgs, copy=True)
    ref = tuple(t.clone() for t in eng.class_map(imgs, k=5))                     # one slice, computed once, left unchanged
    check_outputs(eng, cfg, ref, 5, B5)
    return g, cfg, eng, imgs, fwd, ref


def same(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


def test_class_map_across_slices_and_modes(model):
    g, cfg, eng, imgs, fwd, ref = model
    ncls = cfg.num_classes
    pred = eng.predict(imgs, k=5, copy=True)
    feats = eng.features(imgs, copy=True)
    assert torch.equal(ref[0], pred[0]) and same(ref[1:2], pred[1:2])
    labels = torch.tensor([[3], [0], [ncls], [9], [-1]], dtype=torch.int32, device="cuda")          # two of them outside the classes
    for nslices in (1, 2, 3):                                                    # 5 images: slices of 5; 2 + 3; 1 + 2 + 2
        eng.forward(imgs, nslices=nslices).zero_()
        out = eng.class_map(imgs, k=5, nslices=nslices)
        assert same(out, ref), nslices
        assert torch.equal(eng.last_logits, fwd) and eng.last_logits.data_ptr() == eng._native_buffers(B5, nslices)[1].data_ptr()
        # GIVEN mode: the caller's classes are read, not written; without the head the logits buffer keeps what it held
        lg = eng._native_buffers(B5, nslices)[1]
        lg.fill_(0x5A5A5A5A)
        keep = labels.clone()
        idx, val, tok8, cam32, maps = eng.class_map(imgs, classes=labels, logits=False, nslices=nslices)
        assert val is None and idx.data_ptr() == labels.data_ptr() and torch.equal(labels, keep), nslices
        assert bool((lg == 0x5A5A5A5A).all()), nslices
        assert torch.equal(tok8, ref[2]), nslices
        check_outputs(eng, cfg, (idx, val, tok8, cam32, maps), 1, B5)
        c = cam32.cpu().numpy()
        assert not c[2].any() and not c[4].any() and c[0].any() and np.all(bits(maps[2].cpu().numpy()) == 0x7FC00000)
        # ... and with the head the logits are forward's
        out = eng.class_map(imgs, classes=labels, nslices=nslices, copy=True)
        assert out[1] is None and torch.equal(out[3], cam32) and torch.equal(eng._native_buffers(B5, nslices)[1], fwd), nslices
    # the other entries return what they returned before all of that
    assert torch.equal(eng.forward(imgs), fwd) and same(eng.predict(imgs, k=5), pred) and same(eng.features(imgs), feats)
    # the engine's own buffers, and copies
    a = eng.class_map(imgs)
    b = eng.class_map(imgs, copy=True)
    assert a[2].data_ptr() == eng.class_map(imgs)[2].data_ptr() != b[2].data_ptr() and same(a, b)


def test_headless_class_map_launches_neither_pool_nor_head(model):
    """one slice: the pool's output is the last region of a slice's workspace (al256(B * C + 64) bytes).  Filled beforehand, it keeps
    its bytes without logits — and, as the control that this IS the region, loses them with logits"""
    g, cfg, eng, imgs, fwd, ref = model
    ws, lg = eng._native_buffers(B5, 1)
    tail = (B5 * eng.num_features + 64 + 255) // 256 * 256
    labels = ref[0][:, :2].contiguous()
    pool = ws[ws.numel() - tail:]
    pool.fill_(FILL)
    lg.fill_(0x5A5A5A5A)
    out = eng.class_map(imgs, classes=labels, logits=False)
    torch.cuda.synchronize()
    assert bool((pool == FILL).all()) and bool((lg == 0x5A5A5A5A).all())
    assert torch.equal(out[2], ref[2]) and torch.equal(out[3], ref[3][:, :2]) and same(out[4:], (ref[4][:, :2],))
    eng.class_map(imgs, classes=labels, logits=True)
    torch.cuda.synchronize()
    assert not bool((pool[:B5 * eng.num_features] == FILL).all()) and torch.equal(lg, fwd)
    assert torch.equal(pool[:B5 * eng.num_features].view(torch.int8).reshape(B5, -1), eng.features(imgs)[0])


def test_capture_class_map_replays_on_refilled_images(model):
    g, cfg, eng, _, _, _ = model
    B = 3
    buf = dev(iv.make_images_int8(cfg, B, seed=1))
    replay = eng.capture_class_map(buf, k=5, nstreams=2)
    buf1 = buf.clone()
    classes = torch.zeros(B, 2, dtype=torch.int32, device="cuda")
    headless = eng.capture_class_map(buf1, classes=classes, logits=False, nstreams=1)
    for seed in (61, 62):
        imgs = dev(iv.make_images_int8(cfg, B, seed=seed))
        want = eng.class_map(imgs, k=5, copy=True)
        want_logits = eng.last_logits.clone()
        given = torch.tensor([[seed % 10, 3], [10, 0], [7, 7]], dtype=torch.int32, device="cuda")
        want_given = eng.class_map(imgs, classes=given, logits=False, copy=True)
        buf.copy_(imgs)
        out = replay()
        torch.cuda.synchronize()
        assert same(out, want) and torch.equal(eng._native_buffers(B, 2)[1], want_logits), seed
        buf1.copy_(imgs)
        classes.copy_(given)                                                     # a replay reads the classes as they are then
        out = headless()
        torch.cuda.synchronize()
        assert out[1] is None and out[0].data_ptr() == classes.data_ptr() and same(out[2:], want_given[2:]), seed


# ---------------------------------------------------------------- 4. the runner's refusals
def test_swin_class_map_refusals_launch_nothing(model):
    g, cfg, eng, imgs, fwd, ref = model
    B, k, ncls, C = B5, 5, cfg.num_classes, eng.num_features
    L = (cfg.grid >> (cfg.num_layers - 1)) ** 2
    ws, _ = eng._native_buffers(B, 1)
    sizes = {"images": imgs.numel(), "workspace": ws.numel(), "logits": 4 * B * ncls, "idx": 4 * B * k, "val": 4 * B * k,
             "tok8": B * L * C, "cam32": 4 * B * k * L, "map32": 4 * B * k * L}
    big = max(sizes.values()) + 256
    # twice the largest extent: an array moved onto another one's last bytes still ends inside that one's arena
    arena = {n: torch.full((2 * big,), FILL, dtype=torch.uint8, device="cuda") for n in sizes}
    arena["images"][:imgs.numel()].copy_(imgs.reshape(-1).view(torch.uint8))
    assert all(a.data_ptr() % 256 == 0 for a in arena.values())
    f = eng.h.lib.ivit_swin_class_map
    eng._use_current_stream()
    scale, head_scale = P(eng.class_scale), eng.ptr("head.scale")

    def call(mode=TOPK, k=k, class_scale=scale, head_scale=head_scale, **ptr):
        p = {n: P(arena[n]) for n in sizes}
        p.update(ptr)
        return f(eng.model, p["images"], B, 1, p["workspace"], big, p["logits"], head_scale, mode, k, p["idx"], p["val"], p["tok8"],
                 class_scale, p["cam32"], p["map32"])
    e = lambda: err(eng.h)      # noqa: E731
    assert call(tok8=None) == INV and "tok8" in e()
    assert call(cam32=None) == INV and "cam32" in e()
    assert call(idx=None) == INV and "idx" in e()
    assert call(mode=GIVEN) == INV and "val" in e()                                          # val in GIVEN mode
    assert call(logits=None) == INV and "logits" in e()                                      # NULL logits in TOPK mode
    assert call(head_scale=None) == INV and "head_scale" in e()
    for bad_k in (0, 17, -1, ncls + 1):
        assert call(k=bad_k) == INV and "k" in e(), bad_k
    assert call(mode=GIVEN, val=None, k=17) == INV and "k" in e()
    for mode in (2, -1):
        assert call(mode=mode) == INV and "mode" in e()
    assert call(class_scale=None) == INV and "class_scale" in e() and call(map32=None) == INV and "map32" in e()
    assert call(tok8=P(arena["tok8"], 8)) == INV and "tok8" in e() and "16-byte" in e()
    assert call(cam32=P(arena["cam32"], 2)) == INV and "4-byte" in e() and call(val=P(arena["val"], 2)) == INV and "val" in e()
    assert call(workspace=P(arena["workspace"], 16)) == INV and "workspace" in e()
    assert f(None, P(arena["images"]), B, 1, P(arena["workspace"]), big, None, None, GIVEN, k, P(arena["idx"]), None, P(arena["tok8"]),
             None, P(arena["cam32"]), None) == INV
    # each overlapping pair: the second array put on the first one's start, and on its last bytes
    names = list(sizes)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            for at in (0, (sizes[a] - 4) // 256 * 256):
                assert call(**{b: P(arena[a], at)}) == INV, (a, b, at)
                msg = e()
                assert "overlap" in msg and a in msg and b in msg and "ivit_swin_class_map" in msg, (a, b, msg)
    # GIVEN mode: idx is read, and still judged against everything that is written
    for b in ("workspace", "logits", "tok8", "cam32", "map32"):
        kw = {"idx": P(arena[b])} if b in ("workspace", "logits") else {b: P(arena["idx"])}
        assert call(mode=GIVEN, val=None, **kw) == INV and "overlap" in e() and "idx" in e() and b in e(), (b, e())
    torch.cuda.synchronize()
    for n, a in arena.items():
        if n == "images":
            assert torch.equal(a[:imgs.numel()], imgs.reshape(-1).view(torch.uint8)) and bool((a[imgs.numel():] == FILL).all())
        else:
            assert bool((a == FILL).all()), f"a refused call wrote {n}"
    # the same arguments, nothing wrong with them: accepted, and right
    assert call() == OK, e()
    torch.cuda.synchronize()
    got = lambda n, dt, *shape: arena[n][:sizes[n]].view(dt).reshape(*shape)      # noqa: E731
    assert torch.equal(got("logits", torch.int32, B, ncls), fwd)
    mine = (got("idx", torch.int32, B, k), got("val", torch.float32, B, k), got("tok8", torch.int8, B, L, C),
            got("cam32", torch.int32, B, k, L), got("map32", torch.float32, *ref[4].shape))
    assert same(mine, ref)
    for n in sizes:
        if n not in ("images", "workspace"):
            assert bool((arena[n][sizes[n]:] == FILL).all()), f"wrote behind {n}"
    # map32 and class_scale both absent, GIVEN mode without the head, two slices: cam32 alone
    ws2, _ = eng._native_buffers(B, 2)
    for n in ("logits", "tok8", "cam32", "map32"):
        arena[n].fill_(FILL)
    st = f(eng.model, P(arena["images"]), B, 2, P(ws2), ws2.numel(), None, None, GIVEN, k, P(arena["idx"]), None, P(arena["tok8"]), None,
           P(arena["cam32"]), None)
    assert st == OK, e()
    torch.cuda.synchronize()
    assert torch.equal(got("cam32", torch.int32, B, k, L), ref[3]) and torch.equal(got("tok8", torch.int8, B, L, C), ref[2])
    assert bool((arena["logits"] == FILL).all()) and bool((arena["map32"] == FILL).all())


# ---------------------------------------------------------------- the tool
def test_class_map_tool_writes_what_the_engine_returns(model, tmp_path, capsys, monkeypatch):
    """tools/class_map.py, in this process, on a small file of int8 model inputs"""
    g, cfg, eng, _, _, _ = model
    images = iv.make_images_int8(cfg, 5, seed=81)
    labels = np.array([0, 9, 10, 3, 3], np.int64)                                # one label outside the ten classes
    data, out = str(tmp_path / "data.npz"), str(tmp_path / "maps.npz")
    np.savez(data, images=images, labels=labels)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))
    spec = importlib.util.spec_from_file_location("ivit_tools_class_map", os.path.join(ROOT, "tools", "class_map.py"))
    tool = importlib.util.module_from_spec(spec)
    try:
        spec.loader.exec_module(tool)
    finally:
        sys.modules.pop("evaluate", None)                                        # tools/evaluate.py, which the tool shares its loading with
    base = ["class_map.py", data, "--model", str(g["cfg_name"]), "--golden", os.path.join(ROOT, "tests", "golden", "micro_swin_b2.npz"),
            "--out", out, "--batch", "2"]
    for extra, k, given in ((["--topk", "3"], 3, False), (["--labels"], 1, True)):
        monkeypatch.setattr(sys, "argv", base + extra)
        tool.main()
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert line["n"] == 5 and line["k"] == k and line["given"] is given and line["grid"] == [7, 7]
        z = np.load(out)
        classes = dev(labels.astype(np.int32).reshape(-1, 1)) if given else None
        idx, val, tok8, cam32, maps = eng.class_map(dev(images), k=k, classes=classes, copy=True)
        assert np.array_equal(z["idx"], idx.cpu().numpy()) and z["idx"].dtype == np.int32
        assert z["val"].shape == (5, 0) if given else np.array_equal(bits(z["val"]), bits(val.cpu().numpy()))
        assert z["tok8"].dtype == np.int8 and np.array_equal(z["tok8"], tok8.cpu().numpy()) and z["token_scale"] == np.float32(eng.token_scale_host())
        assert np.array_equal(z["cam32"], cam32.cpu().numpy()) and z["maps"].shape == (5, k, 7, 7)
        assert np.array_equal(bits(z["maps"]), bits(maps.cpu().numpy())) and np.array_equal(z["labels"], labels)
        if given:
            assert not z["cam32"][2].any() and np.isnan(z["maps"][2]).all() and z["cam32"][0].any()
