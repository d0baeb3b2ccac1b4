"""Width 192 on the weights-in-registers GEMM (gemm_ws_qkv_kernel at its K = 192 geometry, csrc/ivit_gemm_ws.h): norm1 + attn.qkv of a
DeiT-Tiny block in one launch with v row-major or transposed, the qkv layer alone, the plain 8-bit layer of Swin's stage 1 and attn.proj
with the identity branch.  Everything is compared with ==: against the CPU oracle's operators (layernorm -> requant 8 -> linear_i8 ->
requant), against the same call on a plan that was not prepared, and through the native ViT runner against the operator chain."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import load_golden, golden_scales

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402

_P = ctypes.c_void_p
K, HH, DH = 192, 3, 64
POISON = 77
S_IN, S_LN = np.float32(7.3e-4), np.float32(0.031)      # norm1: scale of the 16-bit input, scale of its 8-bit output
S_MID, S_FIN, S_RES = np.float32(2e-4), np.float32(3.1e-4), np.float32(2.7e-4)      # proj: qact, residual QuantAct, identity branch


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


def status(H, name, *args):
    return getattr(H.lib, name)(H.h, *args)


# ---------------------------------------------------------------- host data, computed once per (shape, form) and left unchanged
@functools.lru_cache(maxsize=None)
def norm1():
    """LayerNorm constants with negative and small gammas (the seed is one at which N(1, 0.4) gives both among 192 draws)."""
    rng = np.random.default_rng(193)
    wln = rng.normal(1.0, 0.4, K).astype(np.float32)
    assert (wln < 0).any() and (np.abs(wln) < 0.1).any()
    bias_int, sc = iv.freeze.layernorm_constants(wln, rng.normal(0.0, 0.5, K).astype(np.float32))
    return bias_int, sc


@functools.lru_cache(maxsize=None)
def tokens(M):
    """16-bit block input [M, 192] (half of the channels small, row 1 constant: zero variance) and the oracle's norm1 + qact1 of it."""
    from oracle import oracle as orc
    rng = np.random.default_rng(7 * M + 1)
    x16 = rng.integers(-26000, 26000, (M, K)).astype(np.int16)
    x16[:, : K // 2] //= 64
    if M > 1:
        x16[1] = 1234
    bias_int, sc = norm1()
    ln8 = orc.requant(orc.layernorm(x16, float(S_IN), bias_int, sc), orc.dyadic(sc, S_LN), 8).astype(np.int8)
    return x16, ln8


@functools.lru_cache(maxsize=None)
def layer(N, bits, fma, K=K):
    """A frozen QuantLinear K -> N (192 here; tests/test_requant_two_roundings_gpu.py takes the recipe to K = 384 and 1536) with an 8- or
    16-bit QuantAct behind it.  The output scale puts the accumulators' standard deviation at 0.4 of the output range, so that both clamps are reached.  fma = False: channel 5 gets a negative multiplier and a bias of 9.5e6, so
    that |m| * (128 * sum|w| + |bias|) >= 2^53 and the plan cannot take the one-FMA requant (linear_plan_fma_kernel refuses c <= 0)."""
    rng = np.random.default_rng(N * 4 + bits + (0 if fma else 1) + (0 if K == 192 else K))
    w = np.rint(rng.normal(0, 45, (N, K)).clip(-128, 127)).astype(np.int8)
    b = rng.integers(-2 ** 14, 2 ** 14, N).astype(np.int32)
    s_pre = (10 ** rng.uniform(-5.5, -5, N)).astype(np.float32)
    if not fma:
        s_pre[5] = -s_pre[5]
        b[5] = 9500000
    x_std = 74.0 if bits == 16 else 40.0        # uniform int8 rows | norm1's 8-bit output
    acc_std = 45.0 * x_std * np.sqrt(K)
    s_out = np.float32(acc_std * float(np.abs(s_pre).mean()) / (0.4 * 2 ** (bits - 1)))
    return w, b, s_pre, s_out


@functools.lru_cache(maxsize=None)
def qkv_want(M, fma):
    """oracle: qkv Linear + QuantAct(8) of tokens(M)'s norm1 output, [M, 576] int32."""
    from oracle import oracle as orc
    w, b, s_pre, s_out = layer(3 * K, 8, fma)
    return orc.requant(orc.linear_i8(tokens(M)[1], w, b), orc.dyadic(s_pre, s_out), 8)


@functools.lru_cache(maxsize=None)
def res_case(M, N, fma):
    """8-bit context rows, 16-bit identity rows over the whole range, and the oracle's proj -> QuantAct(16) -> residual QuantAct."""
    from oracle import oracle as orc
    rng = np.random.default_rng(M * 5 + N)
    x = rng.integers(-128, 128, (M, K), dtype=np.int8)
    res = rng.integers(-32768, 32768, (M, N)).astype(np.int16)
    res[0, 0::2], res[0, 1::2] = 32767, -32768
    w, b, s_pre, s_out = layer(N, 16, fma)
    t = orc.requant(orc.linear_i8(x, w, b), orc.dyadic(s_pre, s_out), 16)
    want = orc.requant(t, orc.dyadic(S_MID, S_FIN), 16, res.astype(np.int32), orc.dyadic(S_RES, S_FIN))
    return x, res, want


class Plans:
    """Device copies of a layer and two plans of it: one left as created, one prepared (twice: idempotent)."""

    def __init__(self, H, N, bits, fma):
        w, b, s_pre, s_out = layer(N, bits, fma)
        self.keep = [dev(w), dev(b), dev(iv.freeze.dyadic(s_pre, s_out))]
        self.plain = H.linear_plan(P(self.keep[0]), P(self.keep[1]), P(self.keep[2]), N, K)
        self.prepared = H.linear_plan(P(self.keep[0]), P(self.keep[1]), P(self.keep[2]), N, K)
        H.call("ivit_linear_plan_prepare_ws", self.prepared.p)
        H.call("ivit_linear_plan_prepare_ws", self.prepared.p)
        assert self.plain.pipelined_ok and self.plain.single_fma_ok == fma and self.prepared.single_fma_ok == fma

    def close(self):
        self.plain.close()
        self.prepared.close()


@pytest.fixture(scope="module")
def plans(H):
    made = {}

    def get(N, bits, fma):
        if (N, bits, fma) not in made:
            made[(N, bits, fma)] = Plans(H, N, bits, fma)
        return made[(N, bits, fma)]
    yield get
    for p in made.values():
        p.close()


@pytest.fixture(scope="module")
def ln_dev():
    bias_int, sc = norm1()
    return dev(bias_int), dev(sc), dev(iv.freeze.dyadic(sc, S_LN))


def nonvacuous8(want, M):
    if M >= 197:
        assert want.min() == -128 and want.max() == 127 and len(np.unique(want)) > 100


# ---------------------------------------------------------------- 1, 2, 5, 6: the qkv scatter
def run_qkv(H, pl, ln_dev, B, T, ldv, x16=None, a8=None):
    """One launch into poisoned q, k, v buffers with a guard row each; returns (q, k, v) as [B, H, T, 64] host arrays after the checks that
    nothing outside them was written: the guard rows, and in the v^T form the columns t >= T."""
    q, k = (torch.full((B * HH * T + 1, DH), POISON, dtype=torch.int8, device="cuda") for _ in range(2))
    v = torch.full((B * HH * T + 1, DH) if ldv == 0 else (B * HH * DH + 1, ldv), POISON, dtype=torch.int8, device="cuda")
    if x16 is not None:
        bi_d, sc_d, dln = ln_dev
        H.call("ivit_layernorm_linear_i8_qkv_ldv_planned", pl.p, P(x16), float(S_IN), P(bi_d), P(sc_d), P(dln), P(q), P(k), P(v), B, T, HH, DH, ldv)
    else:
        H.call("ivit_linear_i8_qkv_planned", pl.p, P(a8), P(q), P(k), P(v), B, T, HH, DH, ldv)
    out = [t.cpu().numpy() for t in (q, k, v)]
    for o in out:
        assert (o[-1] == POISON).all(), "wrote behind the tensor"
    qh, kh = (o[:-1].reshape(B, HH, T, DH) for o in out[:2])
    if ldv == 0:
        vh = out[2][:-1].reshape(B, HH, T, DH)
    else:
        vt = out[2][:-1].reshape(B, HH, DH, ldv)
        assert (vt[..., T:] == POISON).all(), "v^T columns t >= T were written"
        vh = vt[..., :T].transpose(0, 1, 3, 2)
    return qh, kh, vh


def check_qkv(H, plans, ln_dev, B, T, fma, forms=("alone", "plain", "ln")):
    M, ld = B * T, (T + 15) // 16 * 16
    x16, ln8 = tokens(M)
    want = qkv_want(M, fma)
    nonvacuous8(want, M)
    want = want.reshape(B, T, 3, HH, DH).transpose(2, 0, 3, 1, 4)      # [3][B, H, T, 64]
    pl = plans(3 * K, 8, fma)
    xd, ad = dev(x16), dev(ln8)
    for ldv in (0, ld):
        for form in forms:
            if form == "ln":
                got = run_qkv(H, pl.prepared, ln_dev, B, T, ldv, x16=xd)
            else:
                got = run_qkv(H, pl.prepared if form == "alone" else pl.plain, ln_dev, B, T, ldv, a8=ad)
            for i in range(3):
                bad = int((got[i] != want[i]).sum())
                print(f"B {B} T {T} fma {fma} ldv {ldv} {form} {'qkv'[i]}: mismatches {bad}")
                assert bad == 0, (ldv, form, "qkv"[i], bad)


@pytest.mark.parametrize("fma", [True, False])
@pytest.mark.parametrize("B,T", [(1, 1), (1, 197), (3, 197), (2, 50), (5, 33)])
def test_ws192_qkv_scatter_vs_oracle(H, plans, ln_dev, B, T, fma):
    """q, k, v of a D = 192, three-head layer == the oracle, v row-major (ldv = 0) and transposed (ldv = T rounded up to 16): the qkv layer
    alone on the prepared plan, the same call on the plan as created, and norm1 + qkv in one launch.  Shapes with a ragged last tile, T no
    multiple of 16 or 32 and image boundaries inside a 32-token tile; both requant forms."""
    check_qkv(H, plans, ln_dev, B, T, fma)


@pytest.mark.parametrize("fma", [True, False])
def test_ws192_panel_boundary(H, plans, ln_dev, fma):
    """591 tokens are 19 tiles: on a share of one CU a single workgroup owns them all, more than the 14 tiles of a panel, so it passes
    the barrier in front of its second panel.  Same bytes as on 64 CUs and on the whole device — qkv in every form, and proj + residual."""
    B, T, M = 3, 197, 591
    x, res, want = res_case(M, K, fma)
    pr = plans(K, 16, fma)
    dm, dr = iv.freeze.dyadic(S_MID, S_FIN), iv.freeze.dyadic(S_RES, S_FIN)
    xd, rd = dev(x), dev(res)
    for cus in (1, 64, 0):
        H.set_cu_share(cus)
        try:
            check_qkv(H, plans, ln_dev, B, T, fma, forms=("alone", "ln"))
            out = torch.full((M + 1, K), POISON, dtype=torch.int16, device="cuda")
            H.call("ivit_linear_i8_requant_residual_planned", pr.prepared.p, P(xd), dyv(dm), dyv(dr), P(rd), P(out), M)
            got = out.cpu().numpy()
            assert (got[M] == POISON).all() and np.array_equal(got[:M], want), cus
        finally:
            H.set_cu_share(0)


# ---------------------------------------------------------------- 3: plain 8-bit output
@pytest.mark.parametrize("fma", [True, False])
@pytest.mark.parametrize("M", [1, 49, 784, 3141])
def test_ws192_plain8_vs_oracle(H, plans, ln_dev, M, fma):
    """Swin's qkv layer at C = 192: [M, 576] 8-bit rows in natural order, the layer alone (prepared plan and plan as created) and
    norm1 + layer in one launch, == the oracle."""
    x16, ln8 = tokens(M)
    want = qkv_want(M, fma)
    nonvacuous8(want, M)
    pl = plans(3 * K, 8, fma)
    bi_d, sc_d, dln = ln_dev
    xd, ad = dev(x16), dev(ln8)
    for form in ("alone", "plain", "ln"):
        out = torch.full((M + 1, 3 * K), POISON, dtype=torch.int8, device="cuda")
        if form == "ln":
            H.call("ivit_layernorm_linear_i8_requant_planned", pl.prepared.p, P(xd), float(S_IN), P(bi_d), P(sc_d), P(dln), P(out), M)
        else:
            H.call("ivit_linear_i8_requant_planned", (pl.prepared if form == "alone" else pl.plain).p, P(ad), 8, P(out), M)
        got = out.cpu().numpy()
        bad = int((got[:M] != want).sum())
        print(f"M {M} fma {fma} {form}: mismatches {bad}")
        assert (got[M] == POISON).all() and bad == 0, (form, bad)


# ---------------------------------------------------------------- 4: proj + residual
@pytest.mark.parametrize("fma", [True, False])
@pytest.mark.parametrize("N", [192, 576])
@pytest.mark.parametrize("M", [1, 197, 591, 7000])
def test_ws192_residual_vs_oracle(H, plans, M, N, fma):
    """QuantLinear 192 -> N, QuantAct(16), residual QuantAct with 16-bit identity rows over the whole range: == the oracle on the prepared
    plan and on the plan as created; both 16-bit clamps occur in every case (row 0's identity values are the two extremes)."""
    x, res, want = res_case(M, N, fma)
    print(f"M {M} N {N} fma {fma}: out min {want.min()} max {want.max()}, distinct {len(np.unique(want))}")
    assert want.min() == -32768 and want.max() == 32767
    pl = plans(N, 16, fma)
    dm, dr = iv.freeze.dyadic(S_MID, S_FIN), iv.freeze.dyadic(S_RES, S_FIN)
    xd, rd = dev(x), dev(res)
    for p in (pl.prepared, pl.plain):
        out = torch.full((M + 1, N), POISON, dtype=torch.int16, device="cuda")
        H.call("ivit_linear_i8_requant_residual_planned", p.p, P(xd), dyv(dm), dyv(dr), P(rd), P(out), M)
        got = out.cpu().numpy()
        bad = int((got[:M] != want).sum())
        print(f"  {'prepared' if p is pl.prepared else 'as created'}: mismatches {bad}")
        assert (got[M] == POISON).all() and bad == 0, bad


# ---------------------------------------------------------------- 7: refusals
def test_ws192_refusals(H, plans, ln_dev):
    """Status 3 (unsupported) and nothing written: prepare_ws at K = 256; the LayerNorm entries on a K = 192 plan that was not prepared; the
    qkv scatter at dh = 32; norm2 in the proj launch on a 192 x 192 plan."""
    rng = np.random.default_rng(3)
    w = dev(rng.integers(-128, 128, (256, 256), dtype=np.int8))
    d = dev(iv.freeze.dyadic(np.full(256, 1e-5, np.float32), np.float32(0.02)))
    p256 = H.linear_plan(P(w), None, P(d), 256, 256)
    assert status(H, "ivit_linear_plan_prepare_ws", p256.p) == 3
    msg = H.lib.ivit_last_error(H.h).decode()
    assert "ivit_linear_plan_prepare_ws" in msg and "192" in msg and "384" in msg, msg
    p256.close()

    B, T = 2, 50
    M = B * T
    x16, ln8 = tokens(M)
    xd, ad = dev(x16), dev(ln8)
    bi_d, sc_d, dln = ln_dev
    pq = plans(3 * K, 8, True)
    q, k, v = (torch.full((B * 6 * T + 1, 64), POISON, dtype=torch.int8, device="cuda") for _ in range(3))
    out8 = torch.full((M + 1, 3 * K), POISON, dtype=torch.int8, device="cuda")
    ln = (P(xd), float(S_IN), P(bi_d), P(sc_d), P(dln))
    for ldv in (0, 64):
        assert status(H, "ivit_layernorm_linear_i8_qkv_ldv_planned", pq.plain.p, *ln, P(q), P(k), P(v), B, T, HH, DH, ldv) == 3
        assert "prepare_ws" in H.lib.ivit_last_error(H.h).decode()
        assert status(H, "ivit_layernorm_linear_i8_qkv_ldv_planned", pq.prepared.p, *ln, P(q), P(k), P(v), B, T, 6, 32, ldv) == 3
    assert status(H, "ivit_layernorm_linear_i8_qkv_planned", pq.plain.p, *ln, P(q), P(k), P(v), B, T, HH, DH) == 3
    assert "prepare_ws" in H.lib.ivit_last_error(H.h).decode()
    assert status(H, "ivit_layernorm_linear_i8_qkv_planned", pq.prepared.p, *ln, P(q), P(k), P(v), B, T, 6, 32) == 3
    assert status(H, "ivit_layernorm_linear_i8_requant_planned", pq.plain.p, *ln, P(out8), M) == 3
    assert "prepare_ws" in H.lib.ivit_last_error(H.h).decode()
    pr = plans(K, 16, True)
    x, res, _ = res_case(197, K, True)
    out16 = torch.full((198, K), POISON, dtype=torch.int16, device="cuda")
    a8 = torch.full((198, K), POISON, dtype=torch.int8, device="cuda")
    dm, dr = iv.freeze.dyadic(S_MID, S_FIN), iv.freeze.dyadic(S_RES, S_FIN)
    assert status(H, "ivit_linear_i8_requant_residual_layernorm_planned", pr.prepared.p, P(dev(x)), dyv(dm), dyv(dr), P(dev(res)), P(out16), 197,
                  2.5e-4, P(bi_d), P(sc_d), P(dln), P(a8)) == 3
    torch.cuda.synchronize()
    for t in (q, k, v, out8, out16, a8):
        assert (t == POISON).all()


# ---------------------------------------------------------------- 8, 9: the ViT runner
def _qkv_blocks(eng, batch):
    n = ctypes.c_int(-1)
    assert eng.h.lib.ivit_vit_fused_qkv_blocks(eng.model, batch, ctypes.byref(n)) == 0
    return n.value


@pytest.fixture(scope="module")
def tiny():
    from ivit_amd.engine import ViTEngine
    g = load_golden("deit_tiny_b1.npz")
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    eng = ViTEngine.from_float(cfg, iv.make_vit_weights(cfg, int(g["seed"])), golden_scales(g))
    imgs = np.concatenate([iv.make_images_int8(cfg, 1, int(g["images_seed"])), iv.make_images_int8(cfg, 8, seed=11)])
    d = torch.from_numpy(imgs).cuda()
    ops = eng.forward_ops(d).cpu().numpy()          # norm1, qkv and proj as the separate launches of the operator chain
    return eng, g, cfg, d, ops


def test_ws192_deit_tiny_runner(tiny):
    """DeiT-Tiny through the native runner with norm1 + qkv as one launch in all twelve blocks (the rule has no token-count threshold,
    so at batch 1 too): the fixture's logits at batch 1; at batch 9, whole and in 2 and 4 ragged slices and through a captured graph,
    every image equals the operator chain and image 0 the fixture."""
    eng, g, cfg, d, ops = tiny
    assert not eng._qkv_prepared
    assert _qkv_blocks(eng, 1) == _qkv_blocks(eng, 9) == _qkv_blocks(eng, 256) == cfg.depth == 12
    assert np.array_equal(eng.forward(d[:1].contiguous()).cpu().numpy(), g["logits_int"])
    assert np.array_equal(ops[:1], g["logits_int"])
    for ns in (1, 2, 4):
        got = eng.forward(d, nslices=ns).cpu().numpy()
        assert np.array_equal(got, ops), (ns, int((got != ops).any(axis=1).sum()))
    for ns in (1, 2):
        replay = eng.capture(d, nstreams=ns)
        for _ in range(2):
            got = replay().cpu().numpy()
            assert np.array_equal(got, ops), ("graph", ns, int((got != ops).any(axis=1).sum()))


def test_ws192_fused_qkv_blocks_other_models():
    """The query on the other fixtures: every block of DeiT-S (the path it already takes), none of DeiT-B (D = 768) and of the micro ViT."""
    from ivit_amd.engine import ViTEngine
    for fname, want in (("deit_small_b4.npz", None), ("deit_base_b2.npz", 0), ("micro_vit_b2.npz", 0)):
        g = load_golden(fname)
        cfg = iv.CONFIGS[str(g["cfg_name"])]
        eng = ViTEngine.from_float(cfg, iv.make_vit_weights(cfg, int(g["seed"])), golden_scales(g))
        for batch in (1, 4, 256):
            assert _qkv_blocks(eng, batch) == (cfg.depth if want is None else want), (fname, batch)
        del eng


def test_ws192_two_slices_repeated(tiny):
    """Two slices of batch 8 on the runner's two streams, twenty forwards, each compared image by image with the unsliced result."""
    eng, g, cfg, d, ops = tiny
    d8 = d[:8].contiguous()
    for rep in range(20):
        got = eng.forward(d8, nslices=2).cpu().numpy()
        assert np.array_equal(got, ops[:8]), (rep, np.nonzero((got != ops[:8]).any(axis=1))[0].tolist())
