"""Hidden states on the device, bit for bit, no tolerances.  Operator: ivit_hidden_f32 against `hidden_reference` in both layouts over
the row counts and widths at which the kernels change path (both sides of the 64 x 64 tile's edges, of a 256-thread block of 16-byte
pieces), full-range int16 with both ends, output between guard bands, input unchanged; its refusals launch nothing.  Engines:
ViTEngine / SwinEngine.hidden_states against the REFERENCE's recorded block outputs (micro fixtures) and recorded checksums (DeiT-T,
Swin-T, the window-12 micro Swin), across slice counts, with and without the head, the last-block tap on a model with the
class-token tail, the PatchMerging hazard behind a tapped stage, as a replayed graph; and the runners' refusals, which launch
nothing."""
import ctypes
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, csum, golden_scales, load_golden
from launch_count import captured_nodes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from ivit_amd.predict import hidden_reference  # noqa: E402

_P = ctypes.c_void_p
GUARD_BYTES = 4096
FILL = 0x5A
TOKENS, GRID = _lib.IVIT_HIDDEN_TOKENS, _lib.IVIT_HIDDEN_GRID
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


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def err(h):
    return h.lib.ivit_last_error(h.h).decode()


def _engine(fname):
    g = load_golden(fname)
    if str(g["cfg_name"]) in iv.SWIN_CONFIGS:
        from ivit_amd.swin_engine import SwinEngine
        cfg = iv.SWIN_CONFIGS[str(g["cfg_name"])]
        eng = SwinEngine(cfg, iv.make_swin_weights(cfg, int(g["seed"])), golden_scales(g))
    else:
        from ivit_amd.engine import ViTEngine
        cfg = iv.CONFIGS[str(g["cfg_name"])]
        eng = ViTEngine.from_float(cfg, iv.make_vit_weights(cfg, int(g["seed"])), golden_scales(g))
    return g, cfg, eng


def golden_images(g, cfg):
    return dev(iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"])))


# ---------------------------------------------------------------- 1. the operator
# rows: one; a quarter tile; Swin's 49; both sides of one tile (64) and of two (128); 196.  32 / 33 rows of 64 channels are 256 / 264
# 16-byte pieces: both sides of one block of the stream.  widths: one piece; one tile; a tile and a piece; three tiles
ROWS = (1, 16, 32, 33, 49, 63, 64, 65, 127, 128, 129, 196)
WIDTHS = (8, 64, 72, 192)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("t0", [0, 1])
@pytest.mark.parametrize("layout", ["tokens", "grid"])
def test_hidden_f32_every_bit(H, layout, t0, batch):
    rng = np.random.default_rng(100 * batch + 10 * t0 + (layout == "grid"))
    mode = GRID if layout == "grid" else TOKENS
    for N in ROWS:
        T = N + t0
        for C in WIDTHS:
            q = rng.integers(-32768, 32768, size=(batch, T, C), dtype=np.int64).astype(np.int16)
            q[0, t0, 0], q[-1, T - 1, C - 1], q[-1, T - 1, 0] = -32768, 32767, 0           # both ends, in the first and the last row handed out
            if t0:
                q[:, 0, :] = 32767                                                        # the dropped row: nothing of it may show
            scale = np.float32(rng.uniform(1e-4, 3.0))
            xa, d_x = guarded(q.nbytes)
            d_x.copy_(torch.from_numpy(q.reshape(-1).view(np.uint8)))
            before = xa.clone()
            want = hidden_reference(q, scale, layout, t0)
            out_all, out = guarded(want.nbytes)
            H.call("ivit_hidden_f32", P(d_x), float(scale), batch, T, C, t0, mode, P(out))
            torch.cuda.synchronize()
            assert guards_intact(out_all, want.nbytes), ("wrote outside out", N, C)
            assert torch.equal(xa, before), ("x16 or its surroundings changed", N, C)
            got = out.cpu().numpy().view(np.float32).reshape(want.shape)
            assert np.array_equal(bits(got), bits(want)), (N, C, np.argwhere(bits(got) != bits(want))[:4].tolist())


def test_hidden_f32_refusals_write_nothing(H):
    batch, T, C = 2, 17, 64
    n = batch * T * C
    arena = torch.zeros(8 * n + 4096, dtype=torch.int16, device="cuda")        # x16 and room behind it: no refused call could leave it
    x = arena[:n]
    out_all, out = guarded(4 * n)
    f = H.lib.ivit_hidden_f32
    for args, status, names in (
            ((P(x), 0.01, batch, T, 12, 0, TOKENS, P(out)), UNS, ("C", "multiple of 8")),
            ((P(x), 0.01, batch, T, 12, 0, GRID, P(out)), UNS, ("C", "multiple of 8")),
            ((P(x), 0.01, batch, T, C, T, TOKENS, P(out)), INV, ("t0",)),
            ((P(x), 0.01, batch, T, C, -1, GRID, P(out)), INV, ("t0",)),
            ((P(x), 0.0, batch, T, C, 0, TOKENS, P(out)), INV, ("scale",)),
            ((P(x), -0.5, batch, T, C, 0, TOKENS, P(out)), INV, ("scale",)),
            ((P(x), float("inf"), batch, T, C, 0, GRID, P(out)), INV, ("scale",)),
            ((P(x), float("nan"), batch, T, C, 0, GRID, P(out)), INV, ("scale",)),
            ((P(x), 0.01, batch, T, C, 0, 2, P(out)), INV, ("layout",)),
            ((P(x), 0.01, 0, T, C, 0, TOKENS, P(out)), INV, ("positive",)),
            ((None, 0.01, batch, T, C, 0, TOKENS, P(out)), INV, ("null",)),
            ((P(x), 0.01, batch, T, C, 0, TOKENS, None), INV, ("null",)),
            ((P(x, 2), 0.01, batch, T, C, 0, TOKENS, P(out)), INV, ("x16", "16-byte")),
            ((P(x), 0.01, batch, T, C, 0, GRID, P(out, 4)), INV, ("out", "16-byte")),
            # out over x16: on its start, and on its last 16 bytes
            ((P(x), 0.01, batch, T, C, 0, TOKENS, P(x)), INV, ("overlap", "x16", "out")),
            ((P(x), 0.01, batch, T, C, 1, GRID, P(x, 2 * n - 16)), INV, ("overlap", "x16", "out"))):
        assert f(H.h, *args) == status, (names, err(H))
        for name in names:
            assert name in err(H), (names, err(H))
    assert f(None, P(x), 0.01, batch, T, C, 0, TOKENS, P(out)) == INV
    torch.cuda.synchronize()
    assert bool((out_all == FILL).all()) and int(arena.abs().sum()) == 0, "a refused call wrote"
    # arrays that merely touch are accepted: out directly behind x16
    assert f(H.h, P(x), 0.01, batch, T, C, 0, TOKENS, P(arena, 2 * n)) == OK, err(H)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 2. the ViT engine against the reference's recorded block outputs
def check_hid32(hid16, hid32, eng, sites, layout, class_row):
    """hid32 is the numpy statement of hid16, plane by plane"""
    t0 = 1 if (class_row and layout == "grid") else 0
    for j, i in enumerate(sites):
        want = hidden_reference(hid16[j].cpu().numpy(), np.float32(eng.hidden_scale_host(i)), layout, t0)
        got = hid32[j].cpu().numpy()
        assert got.dtype == np.float32 and got.size == want.size
        assert np.array_equal(bits(got.reshape(want.shape)), bits(want)), (i, layout)


@pytest.mark.parametrize("fname", ["micro_vit_b2.npz", "micro_vit2h_b3.npz"])
def test_vit_hidden_states_equal_the_recorded_sites(fname):
    g, cfg, eng = _engine(fname)
    imgs = golden_images(g, cfg)
    B, T, D = imgs.shape[0], cfg.num_tokens, cfg.embed_dim
    sites = tuple(range(cfg.depth))
    for i in sites:
        assert np.float32(eng.hidden_scale_host(i)) == g[f"scale/blocks.{i}.qact4"], i
    assert eng.hidden_scale_host(-1) == eng.hidden_scale_host(cfg.depth - 1)
    for nslices in (1, 2):                                                       # micro_vit2h_b3: a ragged 2 + 1 split of its three images
        eng.forward(imgs, nslices=nslices).zero_()                               # hidden_states must write the logits buffer itself
        hid16, hid32, logits = eng.hidden_states(imgs, blocks=sites, logits=True, nslices=nslices)
        assert hid16.dtype == torch.int16 and hid16.shape == (cfg.depth, B, T, D) and hid32 is None
        for j, i in enumerate(sites):
            want = g[f"site/blocks.{i}.qact4"]
            assert np.array_equal(hid16[j].cpu().numpy().astype(np.int64), want.astype(np.int64)), (fname, i, nslices)
        assert np.array_equal(logits.cpu().numpy(), g["logits_int"]) and logits.data_ptr() == eng.last_logits.data_ptr()
        for layout in ("tokens", "grid"):
            h16, h32 = eng.hidden_states(imgs, blocks=sites, layout=layout, nslices=nslices)
            gr = cfg.img_size // cfg.patch_size
            assert h32.shape == ((cfg.depth, B, D, gr, gr) if layout == "grid" else (cfg.depth, B, T, D))
            assert torch.equal(h16, hid16)
            check_hid32(h16, h32, eng, sites, layout, True)
    for bad in ((1, 0), (0, 0), (2,), (), (0, -2), 2, -3):
        with pytest.raises(ValueError):
            eng.hidden_states(imgs, blocks=bad)
    with pytest.raises(ValueError):
        eng.hidden_states(imgs, layout="nchw")


def test_vit_last_block_tap_on_a_model_with_the_class_token_tail():
    """the tail computes B rows of the last block; a tap of that block runs it on all rows, the logits are the same integers, and
    forward on the same workspace afterwards is what it was"""
    g, cfg, eng = _engine("micro_vit_b2.npz")
    on = ctypes.c_int(-1)
    assert eng.h.lib.ivit_vit_cls_tail(eng.model, 2, ctypes.byref(on)) == OK and on.value == 1
    imgs = dev(iv.make_images_int8(cfg, 5, seed=31))
    last = cfg.depth - 1
    for nslices in (1, 2):
        fwd = eng.forward(imgs, nslices=nslices, copy=True)
        hid16, _, logits = eng.hidden_states(imgs, blocks=last, logits=True, nslices=nslices, copy=True)
        assert torch.equal(logits, fwd), nslices
        full = eng.hidden_states(imgs, blocks=tuple(range(cfg.depth)), nslices=nslices)[0]
        assert torch.equal(hid16[0], full[last]), nslices
        assert torch.equal(eng.forward(imgs, nslices=nslices), fwd), nslices
        assert eng.h.lib.ivit_vit_cls_tail(eng.model, 5, ctypes.byref(on)) == OK and on.value == 1        # still what forward does
    # the golden batch: the recorded site and the recorded logits from one call
    imgs = golden_images(g, cfg)
    hid16, _, logits = eng.hidden_states(imgs, blocks=-1, logits=True)
    assert np.array_equal(hid16[0].cpu().numpy().astype(np.int64), g[f"site/blocks.{last}.qact4"].astype(np.int64))
    assert np.array_equal(logits.cpu().numpy(), g["logits_int"])


@pytest.mark.parametrize("fname", ["micro_vit_b2.npz", "micro_vit2h_b3.npz"])
def test_vit_taps_without_logits_return_the_same_planes(fname):
    g, cfg, eng = _engine(fname)
    imgs = golden_images(g, cfg)
    B = imgs.shape[0]
    for nslices in (1, 2):
        for blocks in ((0,), (0, cfg.depth - 1)):
            with_head = eng.hidden_states(imgs, blocks=blocks, logits=True, nslices=nslices, copy=True)
            lg = eng._native_buffers(B, nslices)[1]
            lg.fill_(0x5A5A5A5A)                                                 # without the head the logits buffer keeps what it held
            headless = eng.hidden_states(imgs, blocks=blocks, nslices=nslices)
            assert len(headless) == 2 and torch.equal(headless[0], with_head[0]), (blocks, nslices)
            assert bool((lg == 0x5A5A5A5A).all()), (blocks, nslices)
            for j, i in enumerate(blocks):
                assert np.array_equal(headless[0][j].cpu().numpy().astype(np.int64), g[f"site/blocks.{i}.qact4"].astype(np.int64))


def test_deit_tiny_checksums_subset_and_fp32():
    g, cfg, eng = _engine("deit_tiny_b1.npz")
    imgs = golden_images(g, cfg)
    sites = tuple(range(cfg.depth))
    assert cfg.depth == 12
    hid16, hid32, logits = eng.hidden_states(imgs, blocks=sites, layout="tokens", logits=True, copy=True)
    assert np.array_equal(logits.cpu().numpy(), g["logits_int"])
    for i in sites:
        assert csum(hid16[i].cpu().numpy()) == g[f"csum/blocks.{i}.qact4"], i
        assert np.float32(eng.hidden_scale_host(i)) == g[f"scale/blocks.{i}.qact4"], i
    check_hid32(hid16, hid32, eng, sites, "tokens", True)
    sub16, sub32 = eng.hidden_states(imgs, blocks=(3, 11), layout="grid")
    assert sub32.shape == (2, imgs.shape[0], 192, 14, 14)
    assert torch.equal(sub16[0], hid16[3]) and torch.equal(sub16[1], hid16[11])
    check_hid32(sub16, sub32, eng, (3, 11), "grid", True)


# ---------------------------------------------------------------- 3. the Swin engine
def test_swin_stages_equal_the_recorded_sites_and_the_merge_hazard():
    g, cfg, eng = _engine("micro_swin_b2.npz")
    imgs = golden_images(g, cfg)
    B = imgs.shape[0]
    assert cfg.num_layers == 2 and tuple(cfg.depths) == (2, 2)
    fwd = eng.forward(imgs, copy=True)
    assert np.array_equal(fwd.cpu().numpy(), g["logits_int"])
    want = [g[f"site/layers.{li}.blocks.1.qact4"] for li in (0, 1)]
    scales = [g[f"scale/layers.{li}.blocks.1.qact4"] for li in (0, 1)]
    for nslices in (1, 2):
        for layout in (None, "tokens", "grid"):
            hid16, hid32, logits = eng.hidden_states(imgs, stages=(0, 1), layout=layout, logits=True, nslices=nslices)
            assert isinstance(hid16, tuple) and len(hid16) == 2 and torch.equal(logits, fwd)
            for li in (0, 1):
                assert hid16[li].dtype == torch.int16 and tuple(hid16[li].shape) == want[li].shape
                assert np.array_equal(hid16[li].cpu().numpy(), want[li]), (li, nslices, layout)
                assert np.float32(eng.hidden_scale_host(li)) == scales[li]
            if layout is None:
                assert hid32 is None
            else:
                res = [cfg.grid >> li for li in (0, 1)]
                for li in (0, 1):
                    L, C = want[li].shape[1:]
                    assert tuple(hid32[li].shape) == ((B, C, res[li], res[li]) if layout == "grid" else (B, L, C))
                check_hid32(hid16, hid32, eng, (0, 1), layout, False)
        # the PatchMerging hazard: stage 0 alone, its plane must survive the merge's reduction, and the logits are forward's
        eng.forward(imgs, nslices=nslices).zero_()
        hid16, _, logits = eng.hidden_states(imgs, stages=(0,), logits=True, nslices=nslices)
        assert len(hid16) == 1 and np.array_equal(hid16[0].cpu().numpy(), want[0]) and torch.equal(logits, fwd), nslices
        # without the head: the same planes, stage by stage
        for stages in ((0,), (1,), (0, 1)):
            hid16, _ = eng.hidden_states(imgs, stages=stages, nslices=nslices)
            for j, li in enumerate(stages):
                assert np.array_equal(hid16[j].cpu().numpy(), want[li]), (stages, nslices)
        assert torch.equal(eng.forward(imgs, nslices=nslices), fwd)
    for bad in ((1, 0), (0, 0), (2,), ()):
        with pytest.raises(ValueError):
            eng.hidden_states(imgs, stages=bad)


@pytest.mark.parametrize("fname", ["micro_swin_w12_b2.npz", "swin_tiny_b1.npz"])
def test_swin_stages_equal_the_recorded_checksums(fname):
    g, cfg, eng = _engine(fname)
    imgs = golden_images(g, cfg)
    stages = tuple(range(cfg.num_layers))
    slice_counts = (1, 2) if imgs.shape[0] > 1 else (1,)
    planes = None
    for nslices in slice_counts:
        hid16, hid32, logits = eng.hidden_states(imgs, stages=stages, layout="grid", logits=True, nslices=nslices)
        assert np.array_equal(logits.cpu().numpy(), g["logits_int"])
        for li in stages:
            last = cfg.depths[li] - 1
            assert csum(hid16[li].cpu().numpy()) == g[f"csum/layers.{li}.blocks.{last}.qact4"], (li, nslices)
            assert np.float32(eng.hidden_scale_host(li)) == g[f"scale/layers.{li}.blocks.{last}.qact4"], li
        check_hid32(hid16, hid32, eng, stages, "grid", False)
        planes = [t.clone() for t in hid16]
    if imgs.shape[0] == 1:                                                       # one recorded image: two slices on a batch of three fresh ones
        imgs3 = dev(iv.make_images_int8(cfg, 3, seed=77))
        one = [t.clone() for t in eng.hidden_states(imgs3, stages=stages, nslices=1)[0]]
        two = eng.hidden_states(imgs3, stages=stages, nslices=2)[0]
        assert all(torch.equal(a, b) for a, b in zip(one, two))
    assert planes is not None


# ---------------------------------------------------------------- 4. the graph
def test_capture_hidden_states_replays_on_refilled_images():
    g, cfg, eng = _engine("micro_vit2h_b3.npz")
    B = 3
    buf = dev(iv.make_images_int8(cfg, B, seed=1))
    replay = eng.capture_hidden_states(buf, blocks=(0, 1), layout="grid", logits=True, nstreams=2)
    for seed in (61, 62):
        imgs = dev(iv.make_images_int8(cfg, B, seed=seed))
        want16, want32, want_logits = eng.hidden_states(imgs, blocks=(0, 1), layout="grid", logits=True, copy=True)
        buf.copy_(imgs)                                                          # the images overwritten in place
        h16, h32, logits = replay()
        torch.cuda.synchronize()
        assert torch.equal(h16, want16) and torch.equal(h32.view(torch.int32), want32.view(torch.int32)) and torch.equal(logits, want_logits), seed
    gs, cfgs, engs = _engine("micro_swin_b2.npz")
    buf = dev(iv.make_images_int8(cfgs, B, seed=2))
    replay = engs.capture_hidden_states(buf, stages=(0, 1), layout="tokens", nstreams=1)
    for seed in (63, 64):
        imgs = dev(iv.make_images_int8(cfgs, B, seed=seed))
        want16, want32 = engs.hidden_states(imgs, stages=(0, 1), layout="tokens", copy=True)
        buf.copy_(imgs)
        h16, h32 = replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(h16, want16)), seed
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(h32, want32)), seed


# ---------------------------------------------------------------- 5. the runners' refusals and memory contract
def _runner_case(fname, B):
    g, cfg, eng = _engine(fname)
    swin = eng.HIDDEN_SITE == "stage"
    imgs = dev(iv.make_images_int8(cfg, B, seed=53))
    nsites = eng._hidden_sites()
    planes = [eng._hidden_plane(i) for i in range(nsites)]
    n16 = sum(B * T * C for T, C, _ in planes)
    ws, _ = eng._native_buffers(B, 1)
    f = getattr(eng.h.lib, "ivit_swin_hidden_states" if swin else "ivit_vit_hidden_states")
    return g, cfg, eng, imgs, nsites, n16, ws, f, "stages_host" if swin else "blocks_host"


@pytest.mark.parametrize("fname", ["micro_vit2h_b3.npz", "micro_swin_b2.npz"])
def test_hidden_states_refusals_launch_nothing(fname):
    B = 5
    g, cfg, eng, imgs, nsites, n16, ws, f, list_name = _runner_case(fname, B)
    assert nsites == 2
    # one size for all five arrays, the largest extent among them: even a call that were NOT refused would stay inside them
    sizes = {"images": imgs.numel(), "workspace": ws.numel(), "logits": 4 * B * cfg.num_classes, "hid16": 2 * n16, "hid32": 4 * n16}
    big = max(sizes.values()) + 256
    arena = {n: torch.full((big,), FILL, dtype=torch.uint8, device="cuda") for n in sizes}
    arena["images"][:imgs.numel()].copy_(imgs.reshape(-1).view(torch.uint8))
    assert all(a.data_ptr() % 256 == 0 for a in arena.values())
    eng._use_current_stream()

    def call(sites=(0, 1), layout=TOKENS, **ptr):
        p = {n: P(arena[n]) for n in sizes}
        p.update(ptr)
        arr = (ctypes.c_int * max(len(sites), 1))(*sites) if sites is not None else None
        return f(eng.model, p["images"], B, 1, p["workspace"], big, p["logits"], arr, len(sites) if sites is not None else 1,
                 p["hid16"], layout, p["hid32"])
    for sites in ((1, 0), (0, 0), (0, 2), (-1,), (2,), (), (0, 1, 1), None):                  # two sites
        assert call(sites=sites) == INV and list_name in err(eng.h), (sites, err(eng.h))
    assert call(hid16=None) == INV and "hid16" in err(eng.h)
    for layout in (2, -1):
        assert call(layout=layout) == INV and "layout" in err(eng.h)
    assert call(hid16=P(arena["hid16"], 8)) == INV and "hid16" in err(eng.h) and "16-byte" in err(eng.h)
    assert call(hid32=P(arena["hid32"], 4)) == INV and "hid32" in err(eng.h) and "16-byte" in err(eng.h)
    assert call(workspace=P(arena["workspace"], 16)) == INV and "workspace" in err(eng.h)
    # each overlapping pair: the second array put on the first one's start, and on its last bytes (hid16 inside the workspace,
    # hid32 over hid16 among them)
    names = list(sizes)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            for at in (0, (sizes[a] - 16) // 256 * 256):
                assert call(**{b: P(arena[a], at)}) == INV, (a, b, at)
                e = err(eng.h)
                assert "overlap" in e and a in e and b in e and "hidden_states" in e, (a, b, e)
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
    want16, want32, want_logits = eng.hidden_states(imgs, (0, 1), layout="tokens", logits=True)
    got16 = arena["hid16"][:sizes["hid16"]].view(torch.int16)
    got32 = arena["hid32"][:sizes["hid32"]].view(torch.int32)
    flat16 = torch.cat([t.reshape(-1) for t in want16]) if isinstance(want16, tuple) else want16.reshape(-1)
    flat32 = torch.cat([t.reshape(-1) for t in want32]) if isinstance(want32, tuple) else want32.reshape(-1)
    assert torch.equal(got16, flat16) and torch.equal(got32, flat32.view(torch.int32))
    assert torch.equal(arena["logits"][:sizes["logits"]].view(torch.int32).view(B, -1), want_logits)
    assert bool((arena["hid16"][sizes["hid16"]:] == FILL).all()) and bool((arena["hid32"][sizes["hid32"]:] == FILL).all())


@pytest.mark.parametrize("fname", ["micro_vit2h_b3.npz", "micro_swin_b2.npz"])
@pytest.mark.parametrize("layout", [TOKENS, GRID])
def test_hidden_states_write_only_their_outputs(fname, layout):
    """the C entry on the test's own buffers, two ragged slices, no logits: hid16 and hid32 between 4 KiB guard bands, a guard-banded
    logits-sized buffer untouched, the images and their surroundings unchanged"""
    B = 5
    g, cfg, eng, imgs, nsites, n16, ws, f, _ = _runner_case(fname, B)
    swin = eng.HIDDEN_SITE == "stage"
    ws, _ = eng._native_buffers(B, 2)
    t0 = 1 if (layout == GRID and not swin) else 0
    n32 = sum(B * (T - t0) * C for T, C, _ in (eng._hidden_plane(i) for i in range(nsites)))
    img_all, d_img = guarded(imgs.numel())
    d_img.copy_(imgs.reshape(-1).view(torch.uint8))
    before = img_all.clone()
    lg_all, _ = guarded(4 * B * cfg.num_classes)
    a_all, h16 = guarded(2 * n16)
    m_all, h32 = guarded(4 * n32)
    sites = (ctypes.c_int * nsites)(*range(nsites))
    eng._use_current_stream()
    st = f(eng.model, P(d_img), B, 2, P(ws), ws.numel(), None, sites, nsites, P(h16), layout, P(h32))
    assert st == OK, err(eng.h)
    torch.cuda.synchronize()
    assert bool((lg_all == FILL).all()), "logits written without a logits argument"
    assert guards_intact(a_all, h16.numel()) and guards_intact(m_all, h32.numel())
    assert torch.equal(img_all, before), "the images or their surroundings changed"
    name = "grid" if layout == GRID else "tokens"
    want16, want32 = eng.hidden_states(imgs, tuple(range(nsites)), layout=name, nslices=1)
    flat16 = torch.cat([t.reshape(-1) for t in want16]) if isinstance(want16, tuple) else want16.reshape(-1)
    flat32 = torch.cat([t.reshape(-1) for t in want32]) if isinstance(want32, tuple) else want32.reshape(-1)
    assert torch.equal(h16.view(torch.int16), flat16) and torch.equal(h32.view(torch.int32), flat32.view(torch.int32))


# ---------------------------------------------------------------- 6. where a slice ends
# The rows of the table above RunOut::done (csrc/ivit_model.h) that nothing above exercises: a headless tap of the last block alone
# and of a middle block alone (ViT), of stage 0 alone, the last stage with the head, and — the other destination that ends a Swin
# slice early — the class map in GIVEN mode without logits.  (The row with an attention tap AND a hidden tap has no entry.)  Batch 3,
# one slice and a ragged 2 + 1: the integers against the oracle's own planes, tokens and logits on fresh images, the fp32 forms
# against the numpy references, and the launches counted as the nodes of a graph captured around the call.  NODES was recorded from
# the library of commit 5e8798f, where each exit was a hand-written condition: (case, nslices) -> nodes
B3 = 3
NODES = {("vit last", 1): 20, ("vit last", 2): 39, ("vit middle", 1): 12, ("vit middle", 2): 23,
         ("swin stage 0", 1): 20, ("swin stage 0", 2): 39, ("swin stage 1", 1): 42, ("swin stage 1", 2): 83,
         ("swin class map given", 1): 40, ("swin class map given", 2): 79}


def check_nodes(eng, suffix, args, case, nslices):
    n = captured_nodes(eng, suffix, args)
    print("NODES", repr(case), nslices, n)
    assert n == NODES[case, nslices], (case, nslices, n)


@pytest.fixture(scope="module")
def vit3():
    from oracle import oracle as orc
    g, cfg, eng = _engine("micro_vit_b2.npz")
    imgs = iv.make_images_int8(cfg, B3, seed=91)
    cap = {}
    logits, _ = orc.OracleViT(cfg, iv.make_vit_weights(cfg, int(g["seed"])), golden_scales(g)).forward(imgs, capture=cap)
    return cfg, eng, dev(imgs), cap, logits


@pytest.fixture(scope="module")
def swin3():
    from oracle import oracle as orc
    g, cfg, eng = _engine("micro_swin_b2.npz")
    imgs = iv.make_images_int8(cfg, B3, seed=92)                                 # the fixture holds two images: three fresh ones
    cap = {}
    logits, _ = orc.OracleSwin(cfg, iv.make_swin_weights(cfg, int(g["seed"])), golden_scales(g)).forward(imgs, capture=cap)
    return cfg, eng, dev(imgs), cap, logits


@pytest.mark.parametrize("nslices", [1, 2])
@pytest.mark.parametrize("which", ["last", "middle"])
def test_vit_headless_tap_of_one_block_ends_the_slice_behind_it(vit3, which, nslices):
    """the last block alone: the class-token tail is off, the block runs on all rows and the slice ends behind its Mlp launch; a
    middle block alone: the slice ends there.  No final norm, no head: the logits buffer keeps what it held"""
    cfg, eng, imgs, cap, _ = vit3
    i = cfg.depth - 1 if which == "last" else cfg.depth - 2
    assert 0 <= i and (which == "last" or i < cfg.depth - 1)
    lg = eng._native_buffers(B3, nslices)[1]
    lg.fill_(0x5A5A5A5A)
    hid16, hid32 = eng.hidden_states(imgs, blocks=(i,), layout="tokens", nslices=nslices)
    want = np.asarray(cap[f"blocks.{i}.qact4"]).reshape(B3, cfg.num_tokens, cfg.embed_dim)
    assert np.array_equal(hid16[0].cpu().numpy().astype(np.int64), want.astype(np.int64)), (which, nslices)
    check_hid32(hid16, hid32, eng, (i,), "tokens", True)
    assert bool((lg == 0x5A5A5A5A).all()), (which, nslices)
    check_nodes(eng, "_hidden_states", eng._hidden_args(imgs, (i,), "tokens", False, nslices)[0], "vit " + which, nslices)


@pytest.mark.parametrize("nslices", [1, 2])
@pytest.mark.parametrize("stage,logits", [(0, False), (1, True)])
def test_swin_tap_of_one_stage_with_and_without_the_head(swin3, stage, logits, nslices):
    """stage 0 alone, headless: the slice ends behind the stage's last Mlp launch, in front of its merge.  The last stage with the
    head: the whole forward, its last block's output in the caller's plane"""
    cfg, eng, imgs, cap, ref = swin3
    assert cfg.num_layers == 2
    lg = eng._native_buffers(B3, nslices)[1]
    lg.fill_(0x5A5A5A5A)
    out = eng.hidden_states(imgs, stages=(stage,), layout="grid", logits=logits, nslices=nslices)
    L, C, _ = eng._hidden_plane(stage)
    want = np.asarray(cap[f"layers.{stage}.blocks.{cfg.depths[stage] - 1}.qact4"]).reshape(B3, L, C)
    assert np.array_equal(out[0][0].cpu().numpy().astype(np.int64), want.astype(np.int64)), (stage, nslices)
    check_hid32(out[0], out[1], eng, (stage,), "grid", False)
    if logits:
        assert np.array_equal(out[2].cpu().numpy(), ref) and out[2].data_ptr() == lg.data_ptr(), nslices
    else:
        assert bool((lg == 0x5A5A5A5A).all()), nslices
    check_nodes(eng, "_hidden_states", eng._hidden_args(imgs, (stage,), "grid", logits, nslices)[0], f"swin stage {stage}", nslices)


@pytest.mark.parametrize("nslices", [1, 2])
def test_swin_headless_class_map_ends_the_slice_behind_the_final_norm(swin3, nslices):
    """IVIT_CLASSMAP_GIVEN without logits: the final norm writes the caller's tokens and the slice ends — no pool, no head"""
    from ivit_amd.predict import class_map_reference
    cfg, eng, imgs, cap, _ = swin3
    classes = torch.tensor([[1, 0], [2, 9], [0, 3]], dtype=torch.int32, device="cuda")
    assert cfg.num_classes > 9
    lg = eng._native_buffers(B3, nslices)[1]
    lg.fill_(0x5A5A5A5A)
    idx, val, tok8, cam32, maps = eng.class_map(imgs, classes=classes, logits=False, nslices=nslices)
    want = np.asarray(cap["qact2"]).reshape(tuple(tok8.shape))
    assert np.array_equal(tok8.cpu().numpy().astype(np.int64), want.astype(np.int64)), nslices
    o, _, shp = eng.table["head.w"]
    head_w = eng.blob[o:o + int(np.prod(shp))].cpu().numpy().view(np.int8).reshape(shp)
    want_cam, want_map = class_map_reference(want.astype(np.int8), head_w, classes.cpu().numpy(), eng.class_scale.cpu().numpy())
    assert val is None and np.array_equal(cam32.cpu().numpy(), want_cam)
    assert np.array_equal(bits(maps.cpu().numpy().reshape(want_map.shape)), bits(want_map))
    assert bool((lg == 0x5A5A5A5A).all()), nslices
    check_nodes(eng, "_class_map", eng._class_map_args(imgs, 2, classes, False, nslices)[0], "swin class map given", nslices)


# ---------------------------------------------------------------- the tool
def test_hidden_states_tool_writes_what_the_engine_returns(tmp_path, capsys, monkeypatch):
    """tools/hidden_states.py, in this process, on a small file of int8 model inputs"""
    g, cfg, eng = _engine("micro_vit2h_b3.npz")
    images = iv.make_images_int8(cfg, 5, seed=81)
    labels = np.arange(5, dtype=np.int64) % cfg.num_classes
    data, out = str(tmp_path / "data.npz"), str(tmp_path / "hid.npz")
    np.savez(data, images=images, labels=labels)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))
    spec = importlib.util.spec_from_file_location("ivit_tools_hidden_states", os.path.join(ROOT, "tools", "hidden_states.py"))
    tool = importlib.util.module_from_spec(spec)
    try:
        spec.loader.exec_module(tool)
    finally:
        sys.modules.pop("evaluate", None)                                        # tools/evaluate.py, which the tool shares its loading with
    base = ["hidden_states.py", data, "--model", str(g["cfg_name"]), "--golden", os.path.join(ROOT, "tests", "golden", "micro_vit2h_b3.npz"),
            "--out", out, "--batch", "2"]
    for extra, blocks, layout in ((["--blocks", "0,-1", "--layout", "grid"], (0, 1), "grid"), ([], (1,), None)):
        monkeypatch.setattr(sys, "argv", base + extra)
        tool.main()
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert line["n"] == 5 and line["sites"] == list(blocks) and line["layout"] == layout
        z = np.load(out)
        want16, want32 = eng.hidden_states(dev(images), blocks=blocks, layout=layout, copy=True)
        assert np.array_equal(z["sites"], blocks) and np.array_equal(z["labels"], labels)
        assert np.array_equal(bits(z["scales"]), bits(np.asarray([eng.hidden_scale_host(i) for i in blocks], np.float32)))
        for j, i in enumerate(blocks):
            assert z[f"hid16_{i}"].dtype == np.int16 and np.array_equal(z[f"hid16_{i}"], want16[j].cpu().numpy())
            if layout:
                assert np.array_equal(bits(z[f"hid32_{i}"]), bits(want32[j].cpu().numpy()))
            else:
                assert f"hid32_{i}" not in z.files
    monkeypatch.setattr(sys, "argv", base + ["--stages", "0"])
    with pytest.raises(SystemExit):
        tool.main()
