"""Fused Mlp at the widths of Swin-B's stages 0 and 1: width 256 (ivit_mlp_fused_planned on a 256 -> 1024 -> 256 plan, mlp256_kernel)
and width 128 (the stateless ivit_mlp_fused at C = 128, hidden = 512, mlp128_kernel), both on the lock-step body of
csrc/ivit_mlp_body.h.  Bit-exact everywhere: against the CPU oracle's operators, against the three-launch chain the kernels
replace, and through the native Swin runner against the reference's logits.

Operands: the width-192 generator of test_mlp192_gpu.py with both pre-scale exponents moved by -log10(C / 192) / 2 (the
accumulators of a K = C contraction grow like sqrt(C)), so that at either width the hidden tensor reaches -128 and 127 with a
saturated share below half a percent and nothing saturates at 16 bits.  ivit_mlp_plan_create accepts these operands at width 256
as generated (the requant bound is provable): no re-tuning was needed."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden, golden_scales

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402

_P = ctypes.c_void_p
S_GELU, S_G_OUT = np.float32(0.03), np.float32(0.02)
POISON = 0x5555
WIDTHS = (128, 256)


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


def P(t):
    return _P(t.data_ptr())


def dyv(d):
    return _lib.Dyadic(float(d[0, 0]), float(d[0, 1]))


class Case:
    """Operands of one Mlp at width C (host arrays), their device copies, the linear plans of the chain, the ShiftGELU table and — at
    width 256 — the fused plan.  Width 128 has no plan: ivit_mlp_fused takes the operands themselves."""

    def __init__(self, H, C, M, seed, row_scale=False, bias_shift=0):
        rng = np.random.default_rng(seed)
        HD = 4 * C
        self.H, self.C, self.HD, self.M = H, C, HD, M
        self.x = rng.integers(-128, 128, (M, C), dtype=np.int8)
        if row_scale:       # row maxima all over the table: each row of x scaled by U(0, 1)^3, the first 8 rows by 0
            f = rng.uniform(0, 1, M) ** 3
            f[:8] = 0
            self.x = np.rint(self.x * f[:, None]).astype(np.int8)
        self.w1 = rng.integers(-128, 128, (HD, C), dtype=np.int8)
        self.b1 = (rng.integers(-3000, 3000, HD) - bias_shift).astype(np.int32)
        self.w2 = rng.integers(-128, 128, (C, HD), dtype=np.int8)
        self.b2 = rng.integers(-3000, 3000, C).astype(np.int32)
        d = 0.5 * np.log10(C / 192)
        self.s1 = (10 ** rng.uniform(-5.45 - d, -5.05 - d, HD)).astype(np.float32)
        self.s2 = (10 ** rng.uniform(-5.75 - d, -5.35 - d, C)).astype(np.float32)
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
        if C != 128:
            H.call("ivit_mlp_plan_create", self.p1, self.p2, ctypes.byref(self.mp))

    def launch(self, out, dm=None, dr=None):
        """The fused launch's status (the raw C call: refusals are results here, not exceptions)."""
        d, lib, h = self.d, self.H.lib, self.H.h
        dm, dr = dm or dyv(self.dm), dr or dyv(self.dr)
        if self.C == 128:
            return lib.ivit_mlp_fused(h, P(d["x"]), P(d["w1"]), P(d["b1"]), P(d["d1"]), P(self.tab), P(d["w2"]), P(d["b2"]), P(d["d2"]), dm, dr,
                                      P(d["res"]), P(out), self.M, self.C, self.HD)
        return lib.ivit_mlp_fused_planned(h, self.mp, P(d["x"]), P(self.tab), dm, dr, P(d["res"]), P(out), self.M)

    def fused_dev(self):
        """One launch into a poisoned buffer with a canary row behind row M - 1; returns the M rows (device)."""
        out = torch.full((self.M + 1, self.C), POISON, dtype=torch.int16, device="cuda")
        st = self.launch(out)
        assert st == 0, (st, self.H.lib.ivit_last_error(self.H.h).decode())
        assert bool((out[self.M] == POISON).all()), "wrote behind the last row"
        return out[:self.M]

    def fused(self):
        return self.fused_dev().cpu().numpy()

    def chain(self):
        """fc1 + requant -> ShiftGELU table -> fc2 + requant + identity: the three planned launches; returns (hidden, out)."""
        M, C, HD = self.M, self.C, self.HD
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
        if self.mp.value:
            self.H.lib.ivit_mlp_plan_destroy(self.mp)
        self.H.lib.ivit_linear_plan_destroy(self.p1)
        self.H.lib.ivit_linear_plan_destroy(self.p2)


@pytest.mark.parametrize("M", [1, 15, 64, 197, 1000, 160 * 7 + 3, 20011])
@pytest.mark.parametrize("C", WIDTHS)
def test_mlp_swinb_vs_oracle_inputs_a(H, C, M):
    """The operator against the ORACLE's operators (linear_i8 -> requant 8 -> shiftgelu -> requant 8 -> linear_i8 -> requant 16 ->
    requant 16 with the identity), uniform int8 operands.  At M = 20011 the first 200 rows, the last 200 rows and a seeded sample
    of 2000 of the rows between are compared (the operator is row-wise)."""
    c = Case(H, C, M, seed=1000 + M)
    try:
        got = c.fused()
        if M > 5000:
            rng = np.random.default_rng(M)
            rows = np.unique(np.concatenate([np.arange(200), np.arange(M - 200, M), rng.choice(np.arange(200, M - 200), 2000, replace=False)]))
            assert len(rows) >= 2400
        else:
            rows = np.arange(M)
        h, t, o = c.oracle(rows)
        print(f"C {C} M {M}: rows {len(rows)}, hidden min {h.min()} max {h.max()}, saturated {np.mean((h == -128) | (h == 127)):.4f}, "
              f"qact2 |max| {np.abs(t).max()}, distinct outputs {len(np.unique(o))}, mismatches {int((got[rows] != o).sum())}")
        if M >= 64:                     # the test is not vacuous: both ends of the hidden range are reached
            assert h.min() == -128 and h.max() == 127
        if M >= 1000:
            assert len(np.unique(o)) > 10000
        assert np.array_equal(got[rows].astype(np.int32), o), int((got[rows] != o).sum())
    finally:
        c.close()


@pytest.mark.parametrize("bias_shift", [0, 40000])
@pytest.mark.parametrize("C", WIDTHS)
def test_mlp_swinb_vs_oracle_inputs_b(H, C, bias_shift):
    """Inputs B: each row of x scaled by U(0, 1)^3 (the first 8 rows by 0), so that the hidden rows' maxima — each selects one
    of the 256 ShiftGELU table lines — are spread instead of sitting at 127; with the fc1 bias lowered by 40 000 many maxima
    are negative.  Against the oracle, every row."""
    M = 2000
    c = Case(H, C, M, seed=77, row_scale=True, bias_shift=bias_shift)
    try:
        got = c.fused()
        h, t, o = c.oracle(np.arange(M))
        mx = h.max(axis=1)
        print(f"C {C} bias shift {bias_shift}: {len(np.unique(mx))} distinct row maxima in [{mx.min()}, {mx.max()}], {int((mx < 0).sum())} negative, "
              f"mismatches {int((got != o).sum())}")
        assert len(np.unique(mx)) >= 100
        if bias_shift:
            assert (mx < 0).sum() >= 1
        assert np.array_equal(got.astype(np.int32), o), int((got != o).sum())
    finally:
        c.close()


@pytest.mark.parametrize("M", [200704, 50176, 73728, 50191])
@pytest.mark.parametrize("C", WIDTHS)
def test_mlp_swinb_equals_chain_production_geometry(H, C, M):
    """Bit for bit the three-launch chain at the token counts Swin-B produces — 200 704 (stage 0 at 224 px, batch 64), 50 176 (stage 1
    at batch 64, and one of four slices of stage 0), 73 728 (stage 1 at 384 px, batch 32) — and at 50 191, which is not a multiple
    of 16; at the full device and on a share of 64 CUs (ivit_set_cu_share: what the sliced runner gives a slice's handle), six
    launches each into a poisoned buffer with a canary row, every kernel selection the plan accepts (width 128 has no plan and
    one kernel)."""
    c = Case(H, C, M, seed=M + C)
    try:
        h8, ref = c.chain()
        assert int(h8.max()) == 127 and int(h8.min()) == -128
        assert len(torch.unique(ref)) > 10000
        for cus in (0, 64):
            for kernel in ((0, 1) if C != 128 else (None,)):
                if kernel is not None:
                    assert H.lib.ivit_mlp_plan_select(c.mp, kernel) == 0
                H.set_cu_share(cus)
                try:
                    for rep in range(6):
                        got = c.fused_dev()
                        assert torch.equal(got, ref), (cus, kernel, rep, int((got != ref).sum()))
                finally:
                    H.set_cu_share(0)
        if C != 128:
            # the plan has no role-split kernel: refused, and the selection stays what it was
            assert H.lib.ivit_mlp_plan_select(c.mp, 2) == 3
            assert torch.equal(c.fused_dev(), ref)
            assert H.lib.ivit_mlp_plan_select(c.mp, 0) == 0
    finally:
        c.close()


def test_mlp128_wide_multipliers_and_null_bias(H):
    """Width 128 takes its multipliers as the caller holds them, so |z c| < 2^31 is checked by the kernel, per launch: with one fc1
    and one fc2 channel at m = 2^31, 2^-e = 1 it runs on the v_rndne_f64 form and saturates as the unfused operators do
    (ivit_linear_i8_requant / ivit_linear_i8_requant_residual take any multiplier); and biases may be null."""
    M, C, HD = 1123, 128, 512
    c = Case(H, C, M, seed=31)
    try:
        for wide, nobias in ((True, False), (False, True), (True, True)):
            d1, d2 = c.d["d1"].clone(), c.d["d2"].clone()
            if wide:
                d1[5] = torch.tensor([2.0 ** 31, 1.0], dtype=torch.float64)
                d1[300] = torch.tensor([-(2.0 ** 31), 1.0], dtype=torch.float64)
                d2[77] = torch.tensor([2.0 ** 31, 1.0], dtype=torch.float64)
            b1, b2 = (_P(), _P()) if nobias else (P(c.d["b1"]), P(c.d["b2"]))
            h8 = torch.empty(M, HD, dtype=torch.int8, device="cuda")
            g8 = torch.empty_like(h8)
            ref = torch.empty(M, C, dtype=torch.int16, device="cuda")
            H.call("ivit_linear_i8_requant", P(c.d["x"]), P(c.d["w1"]), b1, P(d1), 8, P(h8), M, HD, C)
            H.call("ivit_shiftgelu_requant_lut", P(h8), M, HD, P(c.tab), P(g8))
            H.call("ivit_linear_i8_requant_residual", P(g8), P(c.d["w2"]), b2, P(d2), dyv(c.dm), dyv(c.dr), P(c.d["res"]), P(ref), M, C, HD)
            out = torch.full((M + 1, C), POISON, dtype=torch.int16, device="cuda")
            H.call("ivit_mlp_fused", P(c.d["x"]), P(c.d["w1"]), b1, P(d1), P(c.tab), P(c.d["w2"]), b2, P(d2), dyv(c.dm), dyv(c.dr),
                   P(c.d["res"]), P(out), M, C, HD)
            assert bool((out[M] == POISON).all())
            if wide:                      # the saturated channels are really saturated: the wide form was needed
                hh = h8.cpu().numpy()
                assert (np.abs(hh[:, [5, 300]].astype(np.int32)) >= 127).mean() > 0.99
            assert torch.equal(out[:M], ref), (wide, nobias, int((out[:M] != ref).sum()))
    finally:
        c.close()


def test_mlp_swinb_shapes_and_refusals(H):
    """What the feature adds is accepted — a 256 -> 1024 -> 256 plan, ivit_mlp_fused at (128, 512) — and what it does not build is
    still refused with status 3 (unsupported) and nothing launched: the role-split selection and the LayerNorm-headed launch on a
    width-256 plan, ivit_mlp_fused at (192, 768) and (256, 1024), residual multipliers >= 2^9 at both widths."""
    M = 197
    rng = np.random.default_rng(6)
    big = _lib.Dyadic(1024.0, 1.0)
    cases = {C: Case(H, C, M, seed=5 + C) for C in WIDTHS + (192,)}
    try:
        assert cases[256].mp.value                          # ivit_mlp_plan_create returned 0 (Handle.call raises otherwise)
        for C in WIDTHS:
            c = cases[C]
            out = torch.full((M + 1, C), POISON, dtype=torch.int16, device="cuda")
            assert c.launch(out) == 0
            torch.cuda.synchronize()
            assert not bool((out[:M] == POISON).all()) and bool((out[M] == POISON).all())
            out.fill_(POISON)
            assert c.launch(out, dm=big) == 3
            assert c.launch(out, dr=big) == 3
            torch.cuda.synchronize()
            assert bool((out == POISON).all()), C
        c = cases[256]
        out = torch.full((M + 1, 256), POISON, dtype=torch.int16, device="cuda")
        assert H.lib.ivit_mlp_plan_select(c.mp, 2) == 3
        assert H.lib.ivit_mlp_plan_select(c.mp, 0) == 0 and H.lib.ivit_mlp_plan_select(c.mp, 1) == 0 and H.lib.ivit_mlp_plan_select(c.mp, 0) == 0
        bias_int, sc = iv.freeze.layernorm_constants(rng.normal(1.0, 0.4, 256).astype(np.float32), rng.normal(0.0, 0.5, 256).astype(np.float32))
        bi_d, sc_d = torch.from_numpy(bias_int).cuda(), torch.from_numpy(sc).cuda()
        dln = torch.from_numpy(iv.freeze.dyadic(sc, np.float32(0.031))).cuda()
        scratch = torch.full((M + 1, 256), 77, dtype=torch.int8, device="cuda")
        st = H.lib.ivit_layernorm_mlp_fused_planned(H.h, c.mp, P(c.d["res"]), 2.5e-4, P(bi_d), P(sc_d), P(dln), P(scratch), P(c.tab), dyv(c.dm),
                                                    dyv(c.dr), P(out), M)
        assert st == 3
        # the stateless entry at the widths that have a plan-based kernel instead
        for C in (192, 256):
            c = cases[C]
            o2 = torch.full((M + 1, C), POISON, dtype=torch.int16, device="cuda")
            d = c.d
            st = H.lib.ivit_mlp_fused(H.h, P(d["x"]), P(d["w1"]), P(d["b1"]), P(d["d1"]), P(c.tab), P(d["w2"]), P(d["b2"]), P(d["d2"]), dyv(c.dm),
                                      dyv(c.dr), P(d["res"]), P(o2), M, C, 4 * C)
            assert st == 3
            msg = H.lib.ivit_last_error(H.h).decode()
            assert "96" in msg and "128" in msg, msg
            torch.cuda.synchronize()
            assert bool((o2 == POISON).all()), C
        torch.cuda.synchronize()
        assert bool((out == POISON).all()) and bool((scratch == 77).all())
        # the plan-time refusal names every shape it is built for
        bad = _P()
        assert H.lib.ivit_mlp_plan_create(H.h, cases[256].p2, cases[256].p1, ctypes.byref(bad)) == 3      # 1024 -> 256 -> 1024
        msg = H.lib.ivit_last_error(H.h).decode()
        assert all(s in msg for s in ("384", "1536", "256", "1024", "192", "768")), msg
        assert not bad.value
    finally:
        for c in cases.values():
            c.close()


def _swin_blocks(eng, batch):
    n = (ctypes.c_int * 4)(-1, -1, -1, -1)
    assert eng.h.lib.ivit_swin_fused_mlp_blocks(eng.model, batch, ctypes.byref(n)) == 0
    return list(n)


@pytest.mark.parametrize("fname,B", [("swin_base_b1.npz", 64), ("swin_base_384_b1.npz", 8)])
def test_mlp_swinb_runner(fname, B):
    """Swin-B at 224 px / window 7 and at 384 px / window 12 through the native runner: the fixture's logits at batch 1, both blocks
    of stages 0 (width 128) and 1 (width 256) reported fused and none of stages 2 and 3 (widths 512 and 1024 have no fused kernel);
    at batch B the logits of the operator chain (SwinEngine.forward_ops: the three-launch Mlp) on every image, whole and in four
    slices."""
    from ivit_amd.swin_engine import SwinEngine
    g = load_golden(fname)
    cfg = iv.SWIN_CONFIGS[str(g["cfg_name"])]
    assert cfg.embed_dim == 128 and tuple(cfg.depths) == (2, 2, 18, 2)
    eng = SwinEngine(cfg, iv.make_swin_weights(cfg, int(g["seed"])), golden_scales(g))
    imgs1 = torch.from_numpy(iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"]))).cuda()
    assert np.array_equal(eng.forward(imgs1).cpu().numpy(), g["logits_int"]), fname
    for b in (1, B // 4, B):
        assert _swin_blocks(eng, b) == [2, 2, 0, 0], (fname, b)
    imgs = np.concatenate([iv.make_images_int8(cfg, 1, int(g["images_seed"])), iv.make_images_int8(cfg, B - 1, seed=11)])
    d = torch.from_numpy(imgs).cuda()
    got = eng.forward(d).clone().cpu().numpy()
    assert np.array_equal(got[:1], g["logits_int"])
    sliced = eng.forward(d, nslices=4).clone().cpu().numpy()
    names = []
    orig = eng.h.call
    eng.h.call = lambda name, *a: (names.append(name), orig(name, *a))[1]
    try:
        ops = eng.forward_ops(d).cpu().numpy()
    finally:
        eng.h.call = orig
    assert names.count("ivit_shiftgelu_requant_lut") == sum(cfg.depths) and not any(n.startswith("ivit_mlp_fused") for n in names)
    assert np.array_equal(got, ops), int((got != ops).any(axis=1).sum())
    assert np.array_equal(sliced, ops)


def test_mlp_swinb_leaves_swin_tiny_and_small_alone():
    """Swin-T and Swin-S (widths 96 / 192 / 384 / 768) report what they reported before: every block of stages 0 to 2 fused, none of
    stage 3."""
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
