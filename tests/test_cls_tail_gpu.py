"""The last ViT block's tail on the class-token rows only.  Operator level: the class-token forms of the fused attention write, byte for
byte, rows b*T of what the whole-T entries write, and the identity-row copy (inside that launch, and as ivit_gather_rows_i16) is
rows b*T of the stream.  Runner level: ivit_vit_forward (which applies the rule, ivit_vit_cls_tail) against the per-operator path
that runs the whole last block (ViTEngine.forward_ops) and against the fixtures' logits."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden, golden_scales

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402

_P = ctypes.c_void_p
GUARD8, GUARD16 = 0x5A, 0x5A5A


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


def P(t):
    return _P(t.data_ptr())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dyv(d):
    return _lib.Dyadic(float(d[0, 0]), float(d[0, 1]))


@pytest.mark.parametrize("T", [197, 577, 50, 17])
@pytest.mark.parametrize("B", [1, 3, 37])
def test_cls_attention_equals_rows_of_the_full_entry(H, T, B):
    """All three Shiftmax forms (arithmetic, two-level tables, row table with v^T and with v row-major) — and the arithmetic form with a
    requant multiplier outside the fast range, which takes the exact instantiation — at one scale whose table lines fit 64 entries:
    ctx_cls [B, D] == rows b*T of ctx8 [B, T, D], x_cls [B, D] == rows b*T of x16; one guard row behind each output stays untouched;
    without x16 / x_cls the launch writes ctx_cls alone."""
    scale = np.float32(0.1947)
    tabs = iv.freeze.shiftmax_tables(scale)
    assert tabs is not None and tabs["R"] <= 64
    rng = np.random.default_rng(1000 * T + B)
    Hh, dh = 3, 64
    D = Hh * dh
    ld = (T + 15) // 16 * 16
    q = dev(rng.integers(-128, 128, (B * Hh, T, dh), dtype=np.int8))
    k = dev(rng.integers(-128, 128, (B * Hh, T, dh), dtype=np.int8))
    v = rng.integers(-128, 128, (B * Hh, T, dh), dtype=np.int8)
    vt = np.zeros((B * Hh, dh, ld), np.int8)
    vt[:, :, :T] = v.transpose(0, 2, 1)
    v, vt = dev(v), dev(vt)
    x16 = dev(rng.integers(-32768, 32768, (B * T, D)).astype(np.int16))
    dqk = iv.freeze.dyadic(np.float32(2.2e-4), scale)      # scores spread over the whole int8 range
    dpv = iv.freeze.dyadic(np.float32(2.0 ** -15 * 0.1), np.float32(0.05))
    dqk_slow = _lib.Dyadic(600.0 * 2.0 ** 21, 2.0 ** -21)     # m 2^-e = 600 >= 512: the exact requant (the scores saturate)
    aq, et, cl = dev(tabs["aq"]), dev(tabs["t"]), dev(tabs["cls"])
    rt = torch.empty(256, 64, dtype=torch.float32, device="cuda")
    H.call("ivit_shiftmax_rowtable", P(aq), P(et), P(cl), int(tabs["NC"]), int(tabs["t"].size), int(tabs["dmin"]), P(rt))
    tab_args = (P(aq), P(et), P(cl), int(tabs["NC"]), int(tabs["t"].size), int(tabs["dmin"]))
    forms = {
        "arithmetic": ("ivit_attention_fused", (dyv(dqk), float(scale)), vt, ld),
        "arithmetic, exact requant": ("ivit_attention_fused", (dqk_slow, float(scale)), vt, ld),
        "two-level tables": ("ivit_attention_fused_lut", (dyv(dqk), float(scale)) + tab_args, vt, ld),
        "row table, v^T": ("ivit_attention_fused_rowlut", (dyv(dqk), float(scale), P(rt), int(tabs["dmin"])), vt, ld),
        "row table, v row-major": ("ivit_attention_fused_rowlut", (dyv(dqk), float(scale), P(rt), int(tabs["dmin"])), v, 0),
    }
    want_x = x16.cpu().numpy().reshape(B, T, D)[:, 0]
    for what, (entry, head, vv, ldv) in forms.items():
        full = torch.full((B, T, D), 9, dtype=torch.int8, device="cuda")
        H.call(entry, P(q), P(k), P(vv), *head, dyv(dpv), P(full), B, Hh, T, dh, ldv)
        want = full.cpu().numpy()[:, 0]
        assert len(np.unique(want)) > (20 if "exact" not in what else 1), what
        for with_x in (True, False):
            got = torch.full((B + 1, D), GUARD8, dtype=torch.int8, device="cuda")
            xc = torch.full((B + 1, D), GUARD16, dtype=torch.int16, device="cuda")
            H.call(entry + "_cls", P(q), P(k), P(vv), *head, dyv(dpv), P(got), P(x16) if with_x else None, P(xc) if with_x else None,
                   B, Hh, T, dh, ldv)
            g, x = got.cpu().numpy(), xc.cpu().numpy()
            assert np.array_equal(g[:B], want), (what, with_x, int((g[:B] != want).sum()))
            assert (g[B] == GUARD8).all(), (what, "wrote behind the last context row")
            if with_x:
                assert np.array_equal(x[:B], want_x), what
                assert (x[B] == GUARD16).all(), (what, "wrote behind the last identity row")
            else:
                assert (x == GUARD16).all(), what


def test_cls_attention_argument_checks(H):
    B, Hh, T, dh = 2, 2, 17, 64
    q = torch.zeros(B * Hh, T, dh, dtype=torch.int8, device="cuda")
    vt = torch.zeros(B * Hh, dh, 32, dtype=torch.int8, device="cuda")
    out = torch.zeros(B + 1, Hh * dh, dtype=torch.int8, device="cuda")
    x16 = torch.zeros(B * T, Hh * dh, dtype=torch.int16, device="cuda")
    xc = torch.zeros(B + 1, Hh * dh, dtype=torch.int16, device="cuda")
    one = _lib.Dyadic(1.0, 2.0 ** -10)
    with pytest.raises(_lib.IvitError, match="go together"):
        H.call("ivit_attention_fused_cls", P(q), P(q), P(vt), one, 0.1, one, P(out), P(x16), None, B, Hh, T, dh, 32)
    with pytest.raises(_lib.IvitError, match="16-byte aligned"):
        H.call("ivit_attention_fused_cls", P(q), P(q), P(vt), one, 0.1, one, _P(out.data_ptr() + 4), P(x16), P(xc), B, Hh, T, dh, 32)
    assert H.lib.ivit_attention_fused_cls(H.h, P(q), P(q), P(vt), one, 0.1, one, P(out), P(x16), P(xc), B, Hh, T, 32, 32) == 3     # dh != 64


@pytest.mark.parametrize("T,D", [(197, 384), (577, 768), (50, 192), (17, 64)])
@pytest.mark.parametrize("B", [1, 3, 37])
def test_gather_rows(H, T, D, B):
    rng = np.random.default_rng(T + B)
    x = rng.integers(-32768, 32768, (B * T, D)).astype(np.int16)
    out = torch.full((B + 1, D), GUARD16, dtype=torch.int16, device="cuda")
    H.call("ivit_gather_rows_i16", P(dev(x)), B, D, T * D, P(out))
    got = out.cpu().numpy()
    assert np.array_equal(got[:B], x.reshape(B, T, D)[:, 0])
    assert (got[B] == GUARD16).all(), "wrote behind the last row"


def _cls_tail(eng, batch):
    n = ctypes.c_int(-1)
    assert eng.h.lib.ivit_vit_cls_tail(eng.model, batch, ctypes.byref(n)) == 0
    return n.value


@pytest.mark.parametrize("name", ["deit_tiny_b1.npz", "deit_small_b4.npz", "deit_base_b2.npz", "vit_base_384_b1.npz",
                                  "micro_vit_b2.npz", "micro_vit2h_b3.npz"])
def test_runner_equals_whole_last_block(name):
    """forward (class-token tail) == forward_ops (whole last block, one call per operator) == the fixture's logits; batches 1, 5 and 8
    in 1, 2 and 4 slices (5 images in 2 or 4 slices are ragged: slices of 2 + 3 and of 1 + 1 + 1 + 2, the latter with M = 1 behind the
    attention), and the graph replay whole and in two slices."""
    from ivit_amd.engine import ViTEngine
    g = load_golden(name)
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    eng = ViTEngine.from_float(cfg, iv.make_vit_weights(cfg, int(g["seed"])), golden_scales(g))
    gb = int(g["batch"])
    gold = torch.from_numpy(iv.make_images_int8(cfg, gb, int(g["images_seed"]))).cuda()
    assert np.array_equal(eng.forward(gold).cpu().numpy(), g["logits_int"])
    for B in (1, 5, 8):
        assert _cls_tail(eng, B) == 1
        imgs = np.concatenate([iv.make_images_int8(cfg, gb, int(g["images_seed"])), iv.make_images_int8(cfg, 8, seed=23)])[:B]
        d = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
        ops = eng.forward_ops(d).cpu().numpy()
        n = min(B, gb)
        assert np.array_equal(ops[:n], g["logits_int"][:n])
        for ns in (1, 2, 4):
            got = eng.forward(d, nslices=ns).cpu().numpy()
            assert np.array_equal(got, ops), (name, B, ns, int((got != ops).any(axis=1).sum()))
        for ns in (1, 2):
            replay = eng.capture(d, nstreams=ns)
            for _ in range(2):
                got = replay().cpu().numpy()
                assert np.array_equal(got, ops), (name, B, ns, "graph replay")


def test_runner_deit_small_b256():
    """The headline shape: DeiT-S, 256 random images, every logit row against forward_ops; whole and in two slices."""
    from ivit_amd.engine import ViTEngine
    g = load_golden("deit_small_b4.npz")
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    eng = ViTEngine.from_float(cfg, iv.make_vit_weights(cfg, int(g["seed"])), golden_scales(g))
    assert _cls_tail(eng, 256) == 1
    d = torch.from_numpy(iv.make_images_int8(cfg, 256, seed=31)).cuda()
    ops = eng.forward_ops(d).cpu().numpy()
    got = eng.forward(d, copy=True).cpu().numpy()
    assert np.array_equal(got, ops), int((got != ops).any(axis=1).sum())
    assert np.array_equal(eng.forward(d, nslices=2).cpu().numpy(), ops)
    assert len(np.unique(ops.argmax(axis=1))) > 1
