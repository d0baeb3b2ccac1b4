"""Fused Mlp at width 192 (ivit_mlp_fused_planned on a 192 -> 768 -> 192 plan, mlp192_kernel of csrc/ivit_mlp.h): DeiT-Tiny's blocks and
stage 1 of Swin-T / Swin-S.  Bit-exact everywhere: against the CPU oracle's operators, against the three-launch chain the
kernel replaces, and through the native runners against the reference's logits."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden, golden_scales

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402

_P = ctypes.c_void_p
C, HD = 192, 768
S_GELU, S_G_OUT = np.float32(0.03), np.float32(0.02)
POISON = 0x5555


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


def P(t):
    return _P(t.data_ptr())


def dyv(d):
    return _lib.Dyadic(float(d[0, 0]), float(d[0, 1]))


class Case:
    """Operands of one Mlp at width 192 (host arrays), their device copies, the plans and the ShiftGELU table."""

    def __init__(self, H, M, seed, row_scale=False, bias_shift=0):
        rng = np.random.default_rng(seed)
        self.H, self.M = H, M
        self.x = rng.integers(-128, 128, (M, C), dtype=np.int8)
        if row_scale:       # row maxima all over the table: each row of x scaled by U(0, 1)^3, the first 8 rows by 0
            f = rng.uniform(0, 1, M) ** 3
            f[:8] = 0
            self.x = np.rint(self.x * f[:, None]).astype(np.int8)
        self.w1 = rng.integers(-128, 128, (HD, C), dtype=np.int8)
        self.b1 = (rng.integers(-3000, 3000, HD) - bias_shift).astype(np.int32)
        self.w2 = rng.integers(-128, 128, (C, HD), dtype=np.int8)
        self.b2 = rng.integers(-3000, 3000, C).astype(np.int32)
        self.s1 = (10 ** rng.uniform(-5.45, -5.05, HD)).astype(np.float32)
        self.s2 = (10 ** rng.uniform(-5.75, -5.35, C)).astype(np.float32)
        self.res = rng.integers(-30000, 30000, (M, C)).astype(np.int16)
        self.dm = iv.freeze.dyadic(np.float32(2e-4), np.float32(3.1e-4))
        self.dr = iv.freeze.dyadic(np.float32(2.7e-4), np.float32(3.1e-4))
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.d = {k: up(getattr(self, k)) for k in ("x", "w1", "b1", "w2", "b2", "res")}
        self.d["d1"] = up(iv.freeze.dyadic(self.s1, np.float32(0.012)))
        self.d["d2"] = up(iv.freeze.dyadic(self.s2, np.float32(2e-4)))
        self.tab = torch.empty(65536, dtype=torch.int8, device="cuda")
        H.call("ivit_shiftgelu_build_table", float(S_GELU), dyv(iv.freeze.dyadic(np.float32(S_GELU * 2.0 ** -7), S_G_OUT)), P(self.tab))
        self.p1, self.p2, self.mp = _P(), _P(), _P()
        H.call("ivit_linear_plan_create", P(self.d["w1"]), P(self.d["b1"]), P(self.d["d1"]), HD, C, ctypes.byref(self.p1))
        H.call("ivit_linear_plan_create", P(self.d["w2"]), P(self.d["b2"]), P(self.d["d2"]), C, HD, ctypes.byref(self.p2))
        H.call("ivit_mlp_plan_create", self.p1, self.p2, ctypes.byref(self.mp))

    def fused(self):
        """One launch into a poisoned buffer with a canary row behind row M - 1; returns the M rows."""
        out = torch.full((self.M + 1, C), POISON, dtype=torch.int16, device="cuda")
        self.H.call("ivit_mlp_fused_planned", self.mp, P(self.d["x"]), P(self.tab), dyv(self.dm), dyv(self.dr), P(self.d["res"]), P(out), self.M)
        got = out.cpu().numpy()
        assert (got[self.M] == POISON).all(), "wrote behind the last row"
        return got[:self.M]

    def chain(self):
        """fc1 + requant -> ShiftGELU table -> fc2 + requant + identity: the three planned launches; returns (hidden, out)."""
        M = self.M
        h8 = torch.empty(M, HD, dtype=torch.int8, device="cuda")
        g8 = torch.empty_like(h8)
        ref = torch.empty(M, C, dtype=torch.int16, device="cuda")
        self.H.call("ivit_linear_i8_requant_planned", self.p1, P(self.d["x"]), 8, P(h8), M)
        self.H.call("ivit_shiftgelu_requant_lut", P(h8), M, HD, P(self.tab), P(g8))
        self.H.call("ivit_linear_i8_requant_residual_planned", self.p2, P(g8), dyv(self.dm), dyv(self.dr), P(self.d["res"]), P(ref), M)
        return h8, ref

    def oracle(self, rows):
        """The CPU oracle's operators on the given rows (the operator is row-wise): (hidden int8, qact2 int32, out int32)."""
        from oracle import oracle as orc
        x = self.x[rows]
        h = orc.requant(orc.linear_i8(x, self.w1, self.b1), orc.dyadic(self.s1, np.float32(0.012)), 8)
        g = orc.requant(orc.shiftgelu(h.astype(np.int8), S_GELU).astype(np.int32), orc.dyadic(np.float32(S_GELU * 2.0 ** -7), S_G_OUT), 8)
        t = orc.requant(orc.linear_i8(g.astype(np.int8), self.w2, self.b2), orc.dyadic(self.s2, np.float32(2e-4)), 16)
        o = orc.requant(t, orc.dyadic(np.float32(2e-4), np.float32(3.1e-4)), 16, z_id=self.res[rows].astype(np.int32),
                        dy_id=orc.dyadic(np.float32(2.7e-4), np.float32(3.1e-4)))
        return h, t, o

    def close(self):
        self.H.lib.ivit_mlp_plan_destroy(self.mp)
        self.H.lib.ivit_linear_plan_destroy(self.p1)
        self.H.lib.ivit_linear_plan_destroy(self.p2)


@pytest.mark.parametrize("M", [1, 15, 64, 197, 1000, 160 * 7 + 3, 20011])
def test_mlp192_vs_oracle_inputs_a(H, M):
    """The operator against the ORACLE's operators (linear_i8 -> requant 8 -> shiftgelu -> requant 8 -> linear_i8 -> requant 16 ->
    requant 16 with the identity), uniform int8 operands.  At M = 20011 the oracle's CPU GEMM would take too long for every
    row: the first 200 rows, the last 200 rows and a seeded sample of 2000 of the rows between are compared (the operator is
    row-wise, so the oracle's answer for a row does not depend on the other rows)."""
    c = Case(H, M, seed=1000 + M)
    try:
        got = c.fused()
        if M > 5000:
            rng = np.random.default_rng(M)
            rows = np.unique(np.concatenate([np.arange(200), np.arange(M - 200, M), rng.choice(np.arange(200, M - 200), 2000, replace=False)]))
            assert len(rows) >= 2400
        else:
            rows = np.arange(M)
        h, t, o = c.oracle(rows)
        print(f"M {M}: rows {len(rows)}, hidden min {h.min()} max {h.max()}, saturated {np.mean((h == -128) | (h == 127)):.4f}, "
              f"qact2 |max| {np.abs(t).max()}, distinct outputs {len(np.unique(o))}, mismatches {int((got[rows] != o).sum())}")
        if M >= 64:                     # the test is not vacuous: both ends of the hidden range are reached
            assert h.min() == -128 and h.max() == 127
        if M >= 1000:
            assert len(np.unique(o)) > 10000
        assert np.array_equal(got[rows].astype(np.int32), o), int((got[rows] != o).sum())
    finally:
        c.close()


@pytest.mark.parametrize("bias_shift", [0, 40000])
def test_mlp192_vs_oracle_inputs_b(H, bias_shift):
    """Inputs B: each row of x scaled by U(0, 1)^3 (the first 8 rows by 0), so that the hidden rows' maxima — each selects one
    of the 256 ShiftGELU table lines — are spread instead of sitting at 127; with the fc1 bias lowered by 40 000 many maxima
    are negative.  Against the oracle, every row."""
    M = 2000
    c = Case(H, M, seed=77, row_scale=True, bias_shift=bias_shift)
    try:
        got = c.fused()
        h, t, o = c.oracle(np.arange(M))
        mx = h.max(axis=1)
        print(f"bias shift {bias_shift}: {len(np.unique(mx))} distinct row maxima in [{mx.min()}, {mx.max()}], {int((mx < 0).sum())} negative, "
              f"mismatches {int((got != o).sum())}")
        assert len(np.unique(mx)) >= 100
        if bias_shift:
            assert (mx < 0).sum() >= 1
        assert np.array_equal(got.astype(np.int32), o), int((got != o).sum())
    finally:
        c.close()


@pytest.mark.parametrize("M", [200704, 50432, 50176])
def test_mlp192_equals_chain_production_geometry(H, M):
    """Bit for bit the three-launch chain at the token counts the models produce — 200 704 (Swin-T b256 stage 1), 50 432 (DeiT-T
    b256), 50 176 (one of four Swin slices) — at the full device and on a share of 64 CUs (ivit_set_cu_share: what the sliced
    runner gives a slice's handle), six launches each into a poisoned buffer with a canary row, every kernel the plan has."""
    c = Case(H, M, seed=M)
    try:
        h8, ref = c.chain()
        hh = h8.cpu().numpy()
        assert hh.max() == 127 and hh.min() == -128
        ref = ref.cpu().numpy()
        assert len(np.unique(ref)) > 10000
        for cus in (0, 64):
            for kernel in (0, 1):
                assert H.lib.ivit_mlp_plan_select(c.mp, kernel) == 0
                H.set_cu_share(cus)
                try:
                    for rep in range(6):
                        got = c.fused()
                        assert np.array_equal(got, ref), (cus, kernel, rep, int((got != ref).sum()))
                finally:
                    H.set_cu_share(0)
        # the plan has no role-split kernel: refused, and the selection stays what it was
        assert H.lib.ivit_mlp_plan_select(c.mp, 2) == 3
        assert np.array_equal(c.fused(), ref)
        assert H.lib.ivit_mlp_plan_select(c.mp, 0) == 0
    finally:
        c.close()


def test_mlp192_refusals(H):
    """Shapes the fused kernels are not built for are refused at plan time, residual multipliers out of the fast range at call
    time, and the LayerNorm-headed launch does not exist at this width: status 3 (unsupported), nothing launched."""
    M = 197
    c = Case(H, M, seed=5)
    rng = np.random.default_rng(6)
    keep, plans = [], []

    def lin(N, K):
        w = torch.from_numpy(rng.integers(-128, 128, (N, K), dtype=np.int8)).cuda()
        b = torch.from_numpy(rng.integers(-3000, 3000, N).astype(np.int32)).cuda()
        d = torch.from_numpy(iv.freeze.dyadic((10 ** rng.uniform(-5.9, -5.5, N)).astype(np.float32), np.float32(0.012))).cuda()
        keep.extend([w, b, d])
        p = _P()
        H.call("ivit_linear_plan_create", P(w), P(b), P(d), N, K, ctypes.byref(p))
        plans.append(p)
        return p

    try:
        bad = _P()
        assert H.lib.ivit_mlp_plan_create(H.h, c.p2, c.p1, ctypes.byref(bad)) == 3                      # 768 -> 192 -> 768
        msg = H.lib.ivit_last_error(H.h).decode()
        assert "384" in msg and "1536" in msg and "192" in msg and "768" in msg, msg
        assert H.lib.ivit_mlp_plan_create(H.h, lin(512, 128), lin(128, 512), ctypes.byref(bad)) == 3    # 128 -> 512 -> 128
        assert H.lib.ivit_mlp_plan_create(H.h, lin(3072, 768), lin(768, 3072), ctypes.byref(bad)) == 3  # 768 -> 3072 -> 768
        assert not bad.value
        out = torch.full((M + 1, C), POISON, dtype=torch.int16, device="cuda")
        big = _lib.Dyadic(1024.0, 1.0)
        assert H.lib.ivit_mlp_fused_planned(H.h, c.mp, P(c.d["x"]), P(c.tab), big, dyv(c.dr), P(c.d["res"]), P(out), M) == 3
        assert H.lib.ivit_mlp_fused_planned(H.h, c.mp, P(c.d["x"]), P(c.tab), dyv(c.dm), big, P(c.d["res"]), P(out), M) == 3
        x16 = c.d["res"]
        bias_int, sc = iv.freeze.layernorm_constants(rng.normal(1.0, 0.4, C).astype(np.float32), rng.normal(0.0, 0.5, C).astype(np.float32))
        bi_d, sc_d = torch.from_numpy(bias_int).cuda(), torch.from_numpy(sc).cuda()
        dln = torch.from_numpy(iv.freeze.dyadic(sc, np.float32(0.031))).cuda()
        scratch = torch.full((M + 1, C), 77, dtype=torch.int8, device="cuda")
        st = H.lib.ivit_layernorm_mlp_fused_planned(H.h, c.mp, P(x16), 2.5e-4, P(bi_d), P(sc_d), P(dln), P(scratch), P(c.tab), dyv(c.dm), dyv(c.dr),
                                                    P(out), M)
        assert st == 3
        torch.cuda.synchronize()
        assert (out == POISON).all() and (scratch == 77).all()
    finally:
        c.close()
        for p in plans:
            H.lib.ivit_linear_plan_destroy(p)


def _vit_blocks(eng, batch):
    n = ctypes.c_int(-1)
    assert eng.h.lib.ivit_vit_fused_mlp_blocks(eng.model, batch, ctypes.byref(n)) == 0
    return n.value


def _swin_blocks(eng, batch):
    n = (ctypes.c_int * 4)(-1, -1, -1, -1)
    assert eng.h.lib.ivit_swin_fused_mlp_blocks(eng.model, batch, ctypes.byref(n)) == 0
    return list(n)


def test_mlp192_deit_tiny_runner():
    """DeiT-Tiny (every block at width 192) through the native runner: the fixture's logits at batch 1; at batch 256 the logits of
    the operator chain with the three-launch Mlp (ViTEngine.forward_ops, use_fused_mlp = False) on every image, with all twelve
    blocks reported fused.  forward_ops itself takes the fused branch at this width."""
    from ivit_amd.engine import ViTEngine
    g = load_golden("deit_tiny_b1.npz")
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    eng = ViTEngine.from_float(cfg, iv.make_vit_weights(cfg, int(g["seed"])), golden_scales(g))
    imgs1 = torch.from_numpy(iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"]))).cuda()
    assert np.array_equal(eng.forward(imgs1).cpu().numpy(), g["logits_int"])
    assert 0 <= _vit_blocks(eng, 1) <= cfg.depth             # whatever the token-count rule decides at 197 tokens
    B = 256
    imgs = np.concatenate([iv.make_images_int8(cfg, 1, int(g["images_seed"])), iv.make_images_int8(cfg, B - 1, seed=11)])
    d = torch.from_numpy(imgs).cuda()
    assert _vit_blocks(eng, B) == cfg.depth == 12
    got = eng.forward(d, copy=True).cpu().numpy()
    assert np.array_equal(got[:1], g["logits_int"])
    names = []
    orig = eng.h.call
    eng.h.call = lambda name, *a: (names.append(name), orig(name, *a))[1]
    try:
        ops_fused = eng.forward_ops(d).cpu().numpy()
        assert names.count("ivit_mlp_fused_planned") == cfg.depth and "ivit_shiftgelu_requant_lut" not in names
        del names[:]
        eng.use_fused_mlp = False
        ops_chain = eng.forward_ops(d).cpu().numpy()
        assert names.count("ivit_shiftgelu_requant_lut") == cfg.depth and "ivit_mlp_fused_planned" not in names
    finally:
        eng.h.call = orig
        eng.use_fused_mlp = True
    assert np.array_equal(got, ops_chain), int((got != ops_chain).any(axis=1).sum())
    assert np.array_equal(ops_fused, ops_chain)
    assert np.array_equal(eng.forward(d, nslices=4).cpu().numpy(), ops_chain)


def test_mlp192_swin_runners():
    """Swin-T and Swin-S (stage 1 at width 192) through the native runner: the fixtures' logits at batch 1; Swin-T at batch 256
    equals the operator chain (SwinEngine.forward_ops: three-launch Mlp) on every image, whole and in four slices, with both
    stage-1 blocks reported fused at 256 images and at the 64 images of a slice."""
    from ivit_amd.swin_engine import SwinEngine
    for fname in ("swin_tiny_b1.npz", "swin_small_b1.npz"):
        g = load_golden(fname)
        cfg = iv.SWIN_CONFIGS[str(g["cfg_name"])]
        eng = SwinEngine(cfg, iv.make_swin_weights(cfg, int(g["seed"])), golden_scales(g))
        imgs1 = torch.from_numpy(iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"]))).cuda()
        assert np.array_equal(eng.forward(imgs1).cpu().numpy(), g["logits_int"]), fname
        n1 = _swin_blocks(eng, 1)
        assert n1[0] == cfg.depths[0] and 0 <= n1[1] <= cfg.depths[1], n1
        for B in (256, 64):
            n = _swin_blocks(eng, B)
            assert n[0] == cfg.depths[0] and n[1] == 2 == cfg.depths[1] and n[2] == cfg.depths[2] and n[3] == 0, (fname, B, n)
        if fname != "swin_tiny_b1.npz":
            continue
        B = 256
        imgs = np.concatenate([iv.make_images_int8(cfg, 1, int(g["images_seed"])), iv.make_images_int8(cfg, B - 1, seed=11)])
        d = torch.from_numpy(imgs).cuda()
        got = eng.forward(d).clone().cpu().numpy()
        assert np.array_equal(got[:1], g["logits_int"])
        sliced = eng.forward(d, nslices=4).clone().cpu().numpy()
        ops = eng.forward_ops(d).cpu().numpy()
        assert np.array_equal(got, ops), int((got != ops).any(axis=1).sum())
        assert np.array_equal(sliced, ops)
