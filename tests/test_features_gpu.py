"""Features on the device.  Operator: ivit_features_f32 against `features_reference`, every bit in both modes, over the row widths
at which the kernel changes path (a partial wavefront, a partial last load, exactly one load per lane, the loop) and contents that
stress the sum of squares; its refusals and its memory contract.  Models: features / capture_features of both engines against the
integers the REFERENCE recorded at forward_features' last site, against the operator surface, against forward's logits and
across slice counts; embed; tools/embed.py.

micro_swin_w12_b2.npz records no `site/qact3`, only its checksum: that model is compared through `csum/qact3`, like the full-size
ones."""
import ctypes
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, csum, golden_scales, load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from ivit_amd.predict import embed, features_reference  # noqa: E402
from test_predict_gpu import H, P, _engine, dev  # noqa: E402,F401  (H: the module's handle fixture)

GUARD_BYTES = 4096
FILL = 0x5A
DEQUANT, UNIT = _lib.IVIT_FEATURES_DEQUANT, _lib.IVIT_FEATURES_UNIT


def guarded(nbytes):
    """(whole buffer, payload view): `nbytes` of payload between two 4 KiB guards, everything filled with 0x5A"""
    whole = torch.full((GUARD_BYTES + nbytes + GUARD_BYTES,), FILL, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD_BYTES:GUARD_BYTES + nbytes]


def guards_intact(whole, nbytes):
    w = whole.cpu().numpy()
    return bool(np.all(w[:GUARD_BYTES] == FILL) and np.all(w[GUARD_BYTES + nbytes:] == FILL))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- the kernel alone
def rows_case(batch, dim, seed):
    """random int8 rows; rows 0 .. 5 (as far as the batch goes) are all 127, all -128, zeros, one -128 at the last element, one 127
    at the first, alternating +-127"""
    rng = np.random.default_rng(seed)
    q = rng.integers(-128, 128, size=(batch, dim), dtype=np.int64).astype(np.int8)
    special = np.zeros((6, dim), np.int8)
    special[0], special[1] = 127, -128
    special[3, dim - 1], special[4, 0] = -128, 127
    special[5] = np.where(np.arange(dim) % 2 == 0, 127, -127)
    n = min(batch, 6)
    q[:n] = special[:n]
    return q


def run_features(H, q, scale, mode):
    """ivit_features_f32 on a host array -> float32 [batch, dim]; the guards around `out` and the bytes of feat8 (and around it)
    must stay what they were"""
    B, dim = q.shape
    in_all, d_q = guarded(q.nbytes)
    d_q.copy_(torch.from_numpy(q.reshape(-1).view(np.uint8)))
    before = in_all.clone()
    out_all, out = guarded(4 * B * dim)
    H.call("ivit_features_f32", P(d_q), B, dim, float(scale), mode, P(out))
    torch.cuda.synchronize()
    assert guards_intact(out_all, 4 * B * dim), "wrote outside its output"
    assert torch.equal(in_all, before), "feat8 or its surroundings changed"
    return out.cpu().numpy().view(np.float32).reshape(B, dim)


DIMS = [16, 48, 64, 192, 1008, 1024, 2048]      # partial wavefront (1, 3, 4, 12 lanes), partial last load, one load per lane, the loop
BATCHES = [1, 3, 257]                           # one wavefront of a block, three of four, many blocks with a ragged last one


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("dim", DIMS)
def test_features_f32_every_bit(H, dim, batch):
    scale = np.float32(0.02682777)
    cases = [rows_case(batch, dim, 100 * dim + batch)]
    if batch == 1:                                                # one row at a time: each special row, alone in its launch
        cases += [rows_case(6, dim, 7)[i:i + 1] for i in range(6)]
    for q in cases:
        for mode in (DEQUANT, UNIT):
            got = run_features(H, q, scale, mode)
            want = features_reference(q, scale, mode)
            assert np.array_equal(bits(got), bits(want)), (mode, np.argwhere(bits(got) != bits(want))[:4].tolist())
    q = cases[0]
    unit = run_features(H, q, np.float32(123.5), UNIT)            # the scale is not read in the unit mode
    assert np.array_equal(bits(unit), bits(features_reference(q, scale, UNIT)))
    assert not np.isnan(unit).any()


def test_features_f32_sums_at_squares_and_their_neighbours(H):
    """ss = 64, 63, 67, 127^2 and 2^24 (2048 elements of -128 .. ): a root that is exact, and roots one off an exact one"""
    dim = 64
    rows = np.ones((5, dim), np.int8)
    rows[1, 0] = 0
    rows[2, 1] = 2
    rows[3] = 0
    rows[3, 63] = -127
    rows[4] = 0                                                   # a row of zeros: +0.0 everywhere
    got = run_features(H, rows, 1.0, UNIT)
    assert np.array_equal(bits(got), bits(features_reference(rows, 1.0, UNIT)))
    assert np.all(got[0] == np.float32(0.125)) and got[3, 63] == -1.0 and np.all(bits(got[4]) == 0)
    big = np.full((2, 2048), -128, np.int8)
    big[1, 5] = 127
    got = run_features(H, big, 1.0, UNIT)
    assert np.array_equal(bits(got), bits(features_reference(big, 1.0, UNIT)))
    assert np.all(got[0] == np.float32(-1.0 / np.sqrt(2048.0)))


def test_features_f32_refusals_write_nothing(H):
    q = rows_case(3, 2048, 1)
    wide = torch.zeros(3 * 65552 + 64, dtype=torch.int8, device="cuda")
    d_q = dev(q)
    out_all, out = guarded(4 * 3 * 65552 + 64)
    f = H.lib.ivit_features_f32
    err = lambda: H.lib.ivit_last_error(H.h).decode()      # noqa: E731
    INV, UNS = _lib.IVIT_ERR_INVALID, _lib.IVIT_ERR_UNSUPPORTED
    for args, status, names in (
            ((P(d_q), 3, 24, 0.5, DEQUANT, P(out)), UNS, "dim"),                          # not a multiple of 16
            ((P(wide), 3, 65552, 0.5, UNIT, P(out)), UNS, "dim"),                         # beyond 65536
            ((P(d_q), 3, 2048, 0.5, DEQUANT, ctypes.c_void_p(out.data_ptr() + 4)), INV, "out"),
            ((ctypes.c_void_p(d_q.data_ptr() + 1), 2, 2048, 0.5, DEQUANT, P(out)), INV, "feat8"),
            ((P(d_q), 3, 2048, 0.0, DEQUANT, P(out)), INV, "scale"),
            ((P(d_q), 3, 2048, -0.5, UNIT, P(out)), INV, "scale"),                        # checked in both modes
            ((P(d_q), 3, 2048, float("nan"), DEQUANT, P(out)), INV, "scale"),
            ((P(d_q), 3, 2048, float("nan"), UNIT, P(out)), INV, "scale"),
            ((P(d_q), 3, 2048, float("inf"), DEQUANT, P(out)), INV, "scale"),
            ((P(d_q), 3, 2048, 0.5, 2, P(out)), INV, "mode"),
            ((P(d_q), 3, 2048, 0.5, -1, P(out)), INV, "mode"),
            ((None, 3, 2048, 0.5, DEQUANT, P(out)), INV, "feat8"),
            ((P(d_q), 3, 2048, 0.5, DEQUANT, None), INV, "out"),
            ((P(d_q), -1, 2048, 0.5, DEQUANT, P(out)), INV, "batch"),
            ((P(d_q), 3, 0, 0.5, DEQUANT, P(out)), INV, "dim")):
        assert f(H.h, *args) == status, (names, args[1:5])
        assert names in err(), (names, err())
    assert f(None, P(d_q), 3, 2048, 0.5, DEQUANT, P(out)) == INV
    assert f(H.h, P(d_q), 0, 2048, 0.5, DEQUANT, P(out)) == _lib.IVIT_OK                  # an empty batch launches nothing
    torch.cuda.synchronize()
    assert bool((out_all == FILL).all()), "a refused call wrote"


# ---------------------------------------------------------------- engines against the reference's recorded sites
def _site(g, name):
    return g["site/" + name].reshape(g["site/" + name].shape[0], -1).astype(np.int64) if "site/" + name in g.files else None


@pytest.mark.parametrize("fname", ["micro_vit_b2.npz", "micro_vit2h_b3.npz", "micro_swin_b2.npz", "micro_swin_w12_b2.npz",
                                   "deit_tiny_b1.npz", "swin_tiny_b1.npz"])
def test_engine_features_equal_the_references_last_site(fname):
    g, cfg, eng = _engine(fname)
    site = "qact3" if str(g["cfg_name"]) in iv.SWIN_CONFIGS else "qact2"
    imgs = dev(iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"])))
    B, F = imgs.shape[0], eng.num_features
    assert F == (cfg.num_features if site == "qact3" else cfg.embed_dim) and F % 16 == 0
    assert np.float32(eng.feature_scale_host()) == g["scale/" + site]
    fwd = eng.forward(imgs, copy=True).cpu().numpy()
    assert np.array_equal(fwd, g["logits_int"])
    eng.forward(imgs).zero_()                                                    # features must write the logits buffer itself
    feat8, feat32, logits = eng.features(imgs, logits=True)
    assert feat8.dtype == torch.int8 and feat32.dtype == torch.float32 and feat8.shape == feat32.shape == (B, F)
    assert logits.dtype == torch.int32 and logits.data_ptr() == eng.last_logits.data_ptr()
    f8 = feat8.cpu().numpy()
    want = _site(g, site)
    if want is not None:
        assert fname.startswith("micro") and np.array_equal(f8.astype(np.int64), want)      # every element
    else:
        assert csum(f8) == g["csum/" + site]
    assert np.array_equal(logits.cpu().numpy(), g["logits_int"])
    assert np.array_equal(bits(feat32.cpu().numpy()), bits(features_reference(f8, g["scale/" + site], DEQUANT)))


# ---------------------------------------------------------------- agreement with what exists
MODELS = ["micro_vit_b2.npz", "micro_swin_b2.npz"]
B5 = 5


@pytest.fixture(scope="module", params=MODELS)
def model(request):
    g, cfg, eng = _engine(request.param)
    imgs = dev(iv.make_images_int8(cfg, B5, seed=53))
    return g, cfg, eng, imgs, eng.forward(imgs, copy=True)


def _operator_surface(g, cfg):
    if str(g["cfg_name"]) in iv.SWIN_CONFIGS:
        from ivit_amd.swin_quant import SwinTransformer
        m = SwinTransformer(img_size=cfg.img_size, patch_size=cfg.patch_size, num_classes=cfg.num_classes, embed_dim=cfg.embed_dim,
                            depths=cfg.depths, num_heads=cfg.num_heads, window_size=cfg.window_size, mlp_ratio=cfg.mlp_ratio)
        m.load_float_weights(iv.make_swin_weights(cfg, int(g["seed"])))
    else:
        m = iv.VisionTransformer(img_size=cfg.img_size, patch_size=cfg.patch_size, num_classes=cfg.num_classes,
                                 embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=4)
        m.load_float_weights(iv.make_vit_weights(cfg, int(g["seed"])))
    m.load_act_scales(golden_scales(g))
    iv.freeze_model(m)
    return m


def test_features_across_slices_heads_and_modes(model):
    g, cfg, eng, imgs, fwd = model
    F, scale = eng.num_features, np.float32(eng.feature_scale_host())
    with torch.no_grad():
        x, s = _operator_surface(g, cfg).forward_features(imgs)
    surface = x.reshape(B5, -1).cpu().numpy()
    s = s.detach().cpu().numpy() if hasattr(s, "cpu") else np.asarray(s)
    assert surface.shape == (B5, F) and np.float32(s.reshape(-1)[0]) == scale
    for nslices in (1, 2, 3):                                                    # 5 images: slices of 5; 2 + 3; 1 + 2 + 2
        eng.forward(imgs, nslices=nslices).zero_()
        feat8, feat32 = eng.features(imgs, nslices=nslices)                      # no head: the logits buffer keeps its zeros
        assert int(eng._native_buffers(B5, nslices)[1].abs().sum()) == 0, nslices
        f8 = feat8.cpu().numpy()
        assert np.array_equal(f8.astype(np.int64), surface.astype(np.int64)), nslices
        assert np.array_equal(bits(feat32.cpu().numpy()), bits(features_reference(f8, scale, DEQUANT))), nslices
        h8, h32, logits = eng.features(imgs, normalize=True, logits=True, nslices=nslices, copy=True)
        assert np.array_equal(h8.cpu().numpy(), f8) and torch.equal(logits, fwd), nslices
        assert np.array_equal(bits(h32.cpu().numpy()), bits(features_reference(f8, scale, UNIT))), nslices
    # a second head on the same backbone: the features through ivit_linear_i8 with the head's weights are forward's logits
    acc = torch.zeros(B5, cfg.num_classes, dtype=torch.int32, device="cuda")
    eng.h.call("ivit_linear_i8", P(feat8), eng.ptr("head.w"), eng.ptr("head.b"), P(acc), B5, cfg.num_classes, F)
    assert torch.equal(acc, fwd)
    # the engine's own buffers, and copies
    a = eng.features(imgs)
    b = eng.features(imgs, copy=True)
    assert a[0].data_ptr() == eng.features(imgs)[0].data_ptr() != b[0].data_ptr() and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_capture_features_replays_on_refilled_images(model):
    g, cfg, eng, _, _ = model
    B = 3
    buf = dev(iv.make_images_int8(cfg, B, seed=1))
    replay = eng.capture_features(buf, normalize=True, logits=True, nstreams=2)
    buf1 = buf.clone()
    headless = eng.capture_features(buf1, nstreams=1)
    for seed in (61, 62):
        imgs = dev(iv.make_images_int8(cfg, B, seed=seed))
        want8, want32, want_logits = eng.features(imgs, normalize=True, logits=True, nslices=1, copy=True)
        plain32 = eng.features(imgs, copy=True)[1]
        buf.copy_(imgs)
        feat8, feat32, logits = replay()
        torch.cuda.synchronize()
        assert torch.equal(feat8, want8) and torch.equal(feat32.view(torch.int32), want32.view(torch.int32)), seed
        assert torch.equal(logits, want_logits), seed
        buf1.copy_(imgs)
        f8, f32 = headless()
        torch.cuda.synchronize()
        assert torch.equal(f8, want8) and torch.equal(f32.view(torch.int32), plain32.view(torch.int32)), seed


def test_features_entries_write_only_their_outputs_and_check_first(model):
    """the C entries on guarded buffers of the test's own, eager and as a replayed graph, two slices; then the refusals, which
    launch nothing"""
    g, cfg, eng, imgs, fwd = model
    F, ncls = eng.num_features, cfg.num_classes
    want8, want32, _ = eng.features(imgs, normalize=True, logits=True, copy=True)
    args = list(eng._features_args(imgs, True, True, 2)[0])
    lg_all, lg = guarded(4 * B5 * ncls)
    f8_all, f8 = guarded(B5 * F)
    f32_all, f32 = guarded(4 * B5 * F)
    args[6], args[7], args[10] = P(lg), P(f8), P(f32)

    def check(what):
        torch.cuda.synchronize()
        assert guards_intact(lg_all, 4 * B5 * ncls) and guards_intact(f8_all, B5 * F) and guards_intact(f32_all, 4 * B5 * F), what
        assert torch.equal(f8.view(torch.int8).reshape(B5, F), want8), what
        assert torch.equal(f32.view(torch.int32).reshape(B5, F), want32.view(torch.int32)), what
        assert torch.equal(lg.view(torch.int32).reshape(B5, ncls), fwd), what
        for t in (lg, f8, f32):
            t.fill_(FILL)

    eng._use_current_stream()
    eng._entry("_features", *args)
    check("eager")
    gs, cur = torch.cuda.Stream(), torch.cuda.current_stream()
    torch.cuda.synchronize()
    eng.h.set_stream(gs.cuda_stream)
    graph = ctypes.c_void_p()
    eng._entry("_features_graph_create", *args, ctypes.byref(graph))
    for _ in range(2):
        gs.wait_stream(cur)
        eng.h._check(eng.h.lib.ivit_graph_launch(graph), "ivit_graph_launch")
        cur.wait_stream(gs)
        check("replayed")
    assert eng.h.lib.ivit_graph_destroy(graph) == _lib.IVIT_OK
    eng._use_current_stream()
    # refusals: IVIT_ERR_INVALID, the argument named, nothing written
    entry = getattr(eng.h.lib, eng.PREFIX + "_features")
    err = lambda: eng.h.lib.ivit_last_error(eng.h.h).decode()      # noqa: E731
    for i, value, name in ((7, None, "feat8"), (9, 2, "mode"), (8, 0.0, "scale"), (8, float("nan"), "scale"),
                           (7, ctypes.c_void_p(f8.data_ptr() + 8), "feat8"), (10, ctypes.c_void_p(f32.data_ptr() + 4), "feat32"),
                           (5, 0, eng.PREFIX + "_features: bad arguments / workspace too small"), (1, None, eng.PREFIX + "_features")):
        bad = list(args)
        bad[i] = value
        assert entry(*bad) == _lib.IVIT_ERR_INVALID and name in err(), (name, err())
    bad = list(args)
    bad[8], bad[9] = float("nan"), _lib.IVIT_FEATURES_UNIT                      # a bad scale is refused in the unit mode too ...
    assert entry(*bad) == _lib.IVIT_ERR_INVALID and "scale" in err()
    bad[10] = None                                                               # ... and is of no matter without feat32
    torch.cuda.synchronize()
    assert all(bool((t == FILL).all()) for t in (lg, f8, f32)), "a refused call wrote"
    assert entry(*bad) == _lib.IVIT_OK
    torch.cuda.synchronize()
    assert torch.equal(f8.view(torch.int8).reshape(B5, F), want8) and bool((f32 == FILL).all())


def test_embed_concatenates_per_batch_features(model):
    g, cfg, eng, _, _ = model
    imgs = dev(iv.make_images_int8(cfg, 9, seed=71))
    parts = [imgs[0:4], imgs[4:8], imgs[8:9]]
    for normalize in (True, False):
        want = torch.cat([eng.features(p, normalize=normalize, copy=True)[1] for p in parts])
        out = embed(eng, parts, normalize=normalize) if normalize else embed(eng, [(p, None) for p in parts], normalize=False)
        assert out.device.type == "cuda" and out.shape == (9, eng.num_features)
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    norms = embed(eng, parts).double().norm(dim=1)
    assert bool(((norms - 1).abs() <= 2.0 ** -23).all())


def test_embed_tool_writes_what_the_engine_returns(model, tmp_path, capsys, monkeypatch):
    """tools/embed.py, in this process, on a small file of int8 model inputs"""
    g, cfg, eng, _, _ = model
    fname = f"{g['cfg_name']}_b2.npz"
    assert fname in MODELS
    images = iv.make_images_int8(cfg, 5, seed=81)
    labels = np.arange(5, dtype=np.int64) % cfg.num_classes
    data, out = str(tmp_path / "data.npz"), str(tmp_path / "feats.npz")
    np.savez(data, images=images, labels=labels)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))
    spec = importlib.util.spec_from_file_location("ivit_tools_embed", os.path.join(ROOT, "tools", "embed.py"))
    tool = importlib.util.module_from_spec(spec)
    try:
        spec.loader.exec_module(tool)
    finally:
        sys.modules.pop("evaluate", None)                                        # tools/evaluate.py, which the tool shares its loading with
    for unit in (False, True):
        monkeypatch.setattr(sys, "argv", ["embed.py", data, "--model", str(g["cfg_name"]), "--golden",
                                          os.path.join(ROOT, "tests", "golden", fname), "--out", out, "--batch", "2"] + ["--unit"] * unit)
        tool.main()
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert line["n"] == 5 and line["num_features"] == eng.num_features and line["unit"] is unit
        z = np.load(out)
        want8, want32 = eng.features(dev(images), normalize=unit, copy=True)
        assert np.array_equal(z["feat8"], want8.cpu().numpy()) and np.array_equal(bits(z["features"]), bits(want32.cpu().numpy()))
        assert z["scale"] == np.float32(eng.feature_scale_host()) and np.array_equal(z["labels"], labels)
