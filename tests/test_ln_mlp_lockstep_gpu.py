"""norm2 + qact3 + Mlp + the residual QuantAct as ONE launch of the lock-step kernel at widths 192 and 384
(ivit_layernorm_mlp_lockstep_planned; mlp192ln_kernel / mlp384ln_kernel of csrc/ivit_mlp.h): the LayerNorm's 8-bit rows are computed
straight into the unit's activation tile in LDS and never exist in HBM.  Bit-exact everywhere: against the CPU oracle's operators,
against the two launches it replaces, and through the native runner against the reference's logits."""
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
S_IN, S_LN_OUT, S_FC1_OUT, S_FC2_OUT = np.float32(2.5e-4), np.float32(0.031), np.float32(0.012), np.float32(2e-4)
POISON = 0x5555
NAME = "ivit_layernorm_mlp_lockstep_planned"


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


def P(t):
    return _P(t.data_ptr())


def dyv(d):
    return _lib.Dyadic(float(d[0, 0]), float(d[0, 1]))


class Case:
    """Operands of norm2 + Mlp at width C.  The Mlp's are those of tests/test_mlp192_gpu.py::Case (the fc1 scales follow the width, so
    that the hidden range is reached from LayerNorm's narrower rows); the LayerNorm's those of
    test_gpu_parity.py::test_layernorm_mlp_fused_equals_two_launches: half the channels of x16 divided by 64, weights of both signs, and
    (from 3 rows on) one all-constant row and one row at +-32767.  wide_ln: one channel's multiplier so large that the LayerNorm's
    two-operation 8-bit requant is not provable (|c| (1.2e12 + 1.01 |bias_int|) >= 2^31) and the kernel takes its v_rndne_f64 form.
    tweak: called with the case once its host operands are drawn and before anything is uploaded; it may change them and may put
    (m, e) into rows1 / rows2, rows of fc1's / fc2's per-channel multiplier table written as (m, 2^-e) directly."""

    def __init__(self, H, C, M, seed, wide_ln=False, tweak=None):
        self.H = H
        self.rows1, self.rows2 = {}, {}
        self.host(C, M, seed, wide_ln)
        if tweak is not None:
            tweak(self)
        if H is not None:               # H = None: the host operands and the oracle only (the CPU side of tests/test_mlp_rolesplit_gpu.py)
            self.upload()

    def host(self, C, M, seed, wide_ln):
        rng = np.random.default_rng(seed)
        HD = 4 * C
        self.C, self.HD, self.M = C, HD, M
        self.w1 = rng.integers(-128, 128, (HD, C), dtype=np.int8)
        self.b1 = rng.integers(-3000, 3000, HD).astype(np.int32)
        self.w2 = rng.integers(-128, 128, (C, HD), dtype=np.int8)
        self.b2 = rng.integers(-3000, 3000, C).astype(np.int32)
        self.s1 = (10 ** rng.uniform(-4.9, -4.5, HD) * np.sqrt(192.0 / C)).astype(np.float32)
        self.s2 = (10 ** rng.uniform(-5.75, -5.35, C) * np.sqrt(192.0 / C)).astype(np.float32)
        x16 = rng.integers(-20000, 20000, (M, C)).astype(np.int16)
        x16[:, : C // 2] //= 64
        if M >= 3:
            x16[0] = 1234
            x16[M - 1] = np.where(rng.integers(0, 2, C) > 0, 32767, -32767)
        self.x16 = x16
        wln = rng.normal(1.0, 0.4, C).astype(np.float32) * rng.choice([-1.0, 1.0], C).astype(np.float32)
        self.bias_int, self.sc = iv.freeze.layernorm_constants(wln, rng.normal(0.0, 0.5, C).astype(np.float32))
        self.s_pre = self.sc.copy()             # numerators of norm2's requant multipliers c = s_pre / S_LN_OUT
        if wide_ln:
            self.s_pre[C // 3] = np.float32(2e-3) * S_LN_OUT
            c = float(self.s_pre[C // 3]) / float(S_LN_OUT)
            assert abs(c) * (1.2e12 + 1.01 * abs(float(self.bias_int[C // 3]))) >= 2.0 ** 31
        self.dm = iv.freeze.dyadic(np.float32(2e-4), np.float32(3.1e-4))
        self.dr = iv.freeze.dyadic(np.float32(2.7e-4), np.float32(3.1e-4))

    def upload(self):
        H, C, HD = self.H, self.C, self.HD
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.d = {k: up(getattr(self, k)) for k in ("w1", "b1", "w2", "b2", "x16", "bias_int", "sc")}
        self.d["d1"] = up(self.table(iv.freeze.dyadic(self.s1, S_FC1_OUT), self.rows1))
        self.d["d2"] = up(self.table(iv.freeze.dyadic(self.s2, S_FC2_OUT), self.rows2))
        self.d["dln"] = up(iv.freeze.dyadic(self.s_pre, S_LN_OUT))
        self.tab = torch.empty(65536, dtype=torch.int8, device="cuda")
        H.call("ivit_shiftgelu_build_table", float(S_GELU), dyv(iv.freeze.dyadic(np.float32(S_GELU * 2.0 ** -7), S_G_OUT)), P(self.tab))
        self.p1, self.p2, self.mp = _P(), _P(), _P()
        H.call("ivit_linear_plan_create", P(self.d["w1"]), P(self.d["b1"]), P(self.d["d1"]), HD, C, ctypes.byref(self.p1))
        H.call("ivit_linear_plan_create", P(self.d["w2"]), P(self.d["b2"]), P(self.d["d2"]), C, HD, ctypes.byref(self.p2))
        H.call("ivit_mlp_plan_create", self.p1, self.p2, ctypes.byref(self.mp))

    @staticmethod
    def table(t, rows):
        """a per-channel multiplier table (the library's [n, 2] array or the oracle's) with the rows written directly put in"""
        for ch, (m, e) in rows.items():
            if isinstance(t, np.ndarray):
                t[ch] = (float(m), 2.0 ** -e)
            else:
                t[ch].m, t[ch].r = float(m), 2.0 ** -e
        return t

    def args(self, out, dm=None, dr=None, x16=None):
        d = self.d
        return (self.mp, P(d["x16"]) if x16 is None else x16, float(S_IN), P(d["bias_int"]), P(d["sc"]), P(d["dln"]), P(self.tab),
                dm or dyv(self.dm), dr or dyv(self.dr), P(out), self.M)

    def fused(self):
        """One launch into a poisoned buffer with a canary row behind row M - 1; returns the M rows."""
        out = torch.full((self.M + 1, self.C), POISON, dtype=torch.int16, device="cuda")
        self.H.call(NAME, *self.args(out))
        got = out.cpu().numpy()
        assert (got[self.M] == POISON).all(), "wrote behind the last row"
        return got[:self.M]

    def two_launches(self):
        """ivit_layernorm_requant, then ivit_mlp_fused_planned on the lock-step kernel: (norm2's 8-bit rows, out), on the host."""
        M, C, d = self.M, self.C, self.d
        a8 = torch.empty(M, C, dtype=torch.int8, device="cuda")
        ref = torch.full((M + 1, C), POISON, dtype=torch.int16, device="cuda")
        self.H.call("ivit_layernorm_requant", P(d["x16"]), M, C, C, float(S_IN), P(d["bias_int"]), P(d["sc"]), P(d["dln"]), P(a8))
        assert self.H.lib.ivit_mlp_plan_select(self.mp, 1) == 0
        try:
            self.H.call("ivit_mlp_fused_planned", self.mp, P(a8), P(self.tab), dyv(self.dm), dyv(self.dr), P(d["x16"]), P(ref), M)
        finally:
            assert self.H.lib.ivit_mlp_plan_select(self.mp, 0) == 0
        return a8.cpu().numpy(), ref.cpu().numpy()[:M]

    def oracle(self):
        """The CPU oracle's operators, every row: (norm2's 8-bit rows, hidden int8, out int32)."""
        c = self.chain()
        return c["a"], c["h"], c["o"]

    def chain(self):
        """oracle() with every intermediate: a (norm2's 8-bit rows), h (hidden), g (ShiftGELU + qact1), acc2 (fc2's accumulators
        with the bias), t (qact2, 16 bit), o (the residual QuantAct)."""
        from oracle import oracle as orc
        z = orc.layernorm(self.x16, S_IN, self.bias_int, self.sc)
        a = orc.requant(z, orc.dyadic(self.s_pre, S_LN_OUT), 8)
        h = orc.requant(orc.linear_i8(a.astype(np.int8), self.w1, self.b1), self.table(orc.dyadic(self.s1, S_FC1_OUT), self.rows1), 8)
        return dict(a=a, h=h, **self.from_hidden(h, self.x16))

    def from_hidden(self, h, x16):
        """the chain behind fc1's QuantAct for hidden rows h and their identity rows x16: g, acc2, t, o"""
        from oracle import oracle as orc
        g = orc.requant(orc.shiftgelu(h.astype(np.int8), S_GELU).astype(np.int32), orc.dyadic(np.float32(S_GELU * 2.0 ** -7), S_G_OUT), 8)
        acc2 = orc.linear_i8(g.astype(np.int8), self.w2, self.b2)
        t = orc.requant(acc2, self.table(orc.dyadic(self.s2, S_FC2_OUT), self.rows2), 16)
        return dict(g=g, acc2=acc2, t=t, o=self.residual_act(t, x16))

    @staticmethod
    def residual_act(t, x16):
        """the oracle's residual QuantAct of qact2's rows t with the identity rows x16"""
        from oracle import oracle as orc
        return orc.requant(np.ascontiguousarray(t, np.int32), orc.dyadic(np.float32(2e-4), np.float32(3.1e-4)), 16,
                           z_id=np.ascontiguousarray(x16).astype(np.int32), dy_id=orc.dyadic(np.float32(2.7e-4), np.float32(3.1e-4)))

    def close(self):
        self.H.lib.ivit_mlp_plan_destroy(self.mp)
        self.H.lib.ivit_linear_plan_destroy(self.p1)
        self.H.lib.ivit_linear_plan_destroy(self.p2)


def _vs_oracle(H, C, M, cus, wide_ln=False):
    c = Case(H, C, M, seed=7000 + 13 * C + M, wide_ln=wide_ln)
    try:
        H.set_cu_share(cus)
        try:
            got = c.fused()
        finally:
            H.set_cu_share(0)
        a, h, o = c.oracle()
        print(f"C {C} M {M} cu_share {cus} wide_ln {wide_ln}: norm2 rows in [{a.min()}, {a.max()}], hidden in [{h.min()}, {h.max()}], "
              f"distinct outputs {len(np.unique(o))}, mismatches {int((got != o).sum())}")
        if M >= 80:                     # not vacuous: both ends of the hidden range, and of norm2's, are reached
            assert h.min() == -128 and h.max() == 127
            assert a.min() == -128 and a.max() == 127
        assert np.array_equal(got.astype(np.int32), o), int((got != o).sum())
    finally:
        c.close()


# width 192, 1123 rows = 71 tiles: on 7 CUs 14 workgroups of 5 or 6 tiles (units of 5 | 3 + 3), on 1 CU two workgroups of 35 and 36
# tiles (seven units of 5; eight of 4 or 5), the last tile ragged.  Width 384 on 7 CUs: 550 rows = 35 tiles, 9 units of 4 take two
# rounds round-robin and one balanced (7 workgroups of one 5-tile unit); 600 rows = 38 tiles, 10 units, two rounds either way:
# round-robin, the next unit of a workgroup 7 units on
@pytest.mark.parametrize("C,M,cus", [(192, m, 0) for m in (1, 15, 16, 17, 80, 81, 197, 1123)] + [(192, 1123, 7), (192, 1123, 1)] +
                         [(384, m, 0) for m in (1, 17, 81, 256, 550, 600)] + [(384, 550, 7), (384, 600, 7)])
def test_ln_mlp_lockstep_vs_oracle(H, C, M, cus):
    """The launch against the ORACLE's operators (layernorm -> requant 8 per channel -> linear_i8 -> requant 8 -> shiftgelu -> requant 8
    -> linear_i8 -> requant 16 -> requant 16 with the identity), every row, into a poisoned buffer with a canary row."""
    _vs_oracle(H, C, M, cus)


@pytest.mark.parametrize("C,M,cus", [(192, 1123, 7), (384, 600, 7)])
def test_ln_mlp_lockstep_vs_oracle_wide_requant(H, C, M, cus):
    """The same with one LayerNorm channel whose multiplier is out of the two-operation requant's range: the whole launch takes the
    v_rndne_f64 form (ln_stage_constants answers false)."""
    _vs_oracle(H, C, M, cus, wide_ln=True)


@pytest.mark.parametrize("C,M", [(192, 197), (192, 50432), (384, 256), (384, 20480)])
def test_ln_mlp_lockstep_equals_two_launches(H, C, M):
    """Bit for bit ivit_layernorm_requant followed by ivit_mlp_fused_planned on the lock-step kernel, at the models' own token counts
    (DeiT-T b1 and b256; the class-token tail of DeiT-S b256 and one unit per CU), at the full device and on a share of 64 CUs, three
    launches each into a poisoned buffer with a canary row."""
    c = Case(H, C, M, seed=M + C)
    try:
        a8, ref = c.two_launches()
        assert a8.min() == -128 and a8.max() == 127
        assert len(np.unique(ref)) > (10000 if M > 1000 else 1000)
        for cus in (0, 64):
            H.set_cu_share(cus)
            try:
                for rep in range(3):
                    got = c.fused()
                    assert np.array_equal(got, ref), (cus, rep, int((got != ref).sum()))
            finally:
                H.set_cu_share(0)
        # whatever the plan is pinned to, the entry runs the lock-step kernel
        for kernel in ((1, 2) if C == 384 else (1,)):
            assert H.lib.ivit_mlp_plan_select(c.mp, kernel) == 0
            got = c.fused()
            assert H.lib.ivit_mlp_plan_select(c.mp, 0) == 0
            assert np.array_equal(got, ref), kernel
    finally:
        c.close()


def test_ln_mlp_lockstep_refusals(H):
    """A width the head is not built for and residual multipliers out of the fast range: status 3; the output aliasing the input: status 1.
    Nothing launched: the buffers keep their poison."""
    M = 197
    c256, c = Case(H, 256, M, seed=3), Case(H, 192, M, seed=4)
    try:
        out = torch.full((M + 1, 256), POISON, dtype=torch.int16, device="cuda")
        assert getattr(H.lib, NAME)(H.h, *c256.args(out)) == 3
        msg = H.lib.ivit_last_error(H.h).decode()
        assert "192" in msg and "384" in msg, msg
        torch.cuda.synchronize()
        assert (out == POISON).all()
        out = torch.full((M + 1, 192), POISON, dtype=torch.int16, device="cuda")
        big = _lib.Dyadic(1024.0, 1.0)
        assert getattr(H.lib, NAME)(H.h, *c.args(out, dm=big)) == 3
        assert getattr(H.lib, NAME)(H.h, *c.args(out, dr=big)) == 3
        torch.cuda.synchronize()
        assert (out == POISON).all()
        x = c.d["x16"].clone()
        assert getattr(H.lib, NAME)(H.h, *c.args(x, x16=P(x))) == 1
        torch.cuda.synchronize()
        assert torch.equal(x, c.d["x16"])
        assert getattr(H.lib, NAME)(H.h, *c.args(out)) == 0          # and the same arguments, not aliased, run
        torch.cuda.synchronize()
        assert (out[M] == POISON).all() and not (out[:M] == POISON).all()
    finally:
        c256.close()
        c.close()


def _ln_mlp_blocks(eng, batch):
    n = ctypes.c_int(-1)
    assert eng.h.lib.ivit_vit_fused_ln_mlp_blocks(eng.model, batch, ctypes.byref(n)) == 0
    return n.value


def _engine(name):
    from ivit_amd.engine import ViTEngine
    g = load_golden(name)
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    return g, cfg, ViTEngine.from_float(cfg, iv.make_vit_weights(cfg, int(g["seed"])), golden_scales(g))


@pytest.mark.parametrize("name,batches,want", [("deit_tiny_b1.npz", (1, 256), 12), ("deit_small_b4.npz", (4, 256), 12),
                                               ("deit_base_b2.npz", (2, 256), 0), ("micro_vit_b2.npz", (2,), 0),
                                               ("micro_vit2h_b3.npz", (3,), 0)])
def test_fused_ln_mlp_blocks(name, batches, want):
    """Blocks whose norm2 + Mlp is one launch, through either LayerNorm-headed entry (the last block at its tail's row count): all
    twelve at widths 192 and 384 at every batch, none at the other widths."""
    g, cfg, eng = _engine(name)
    for B in batches:
        assert _ln_mlp_blocks(eng, B) == want, (name, B)
    assert eng.h.lib.ivit_vit_fused_ln_mlp_blocks(eng.model, 0, ctypes.byref(ctypes.c_int())) == 1
    assert eng.h.lib.ivit_vit_fused_ln_mlp_blocks(eng.model, 1, None) == 1


@pytest.mark.parametrize("name,B,ns", [("deit_tiny_b1.npz", 1, 1), ("deit_tiny_b1.npz", 3, 2), ("deit_small_b4.npz", 2, 1)])
def test_runner_through_lockstep_ln_mlp(name, B, ns):
    """ViTEngine.forward (the native runner: norm2 + Mlp of every block through the new entry at these shapes) == forward_ops with the
    switch off (LayerNorm + ivit_mlp_fused_planned) == forward_ops with it on (the new entry, once per block); a captured graph replays
    to the same logits twice; the fixture's logits hold."""
    g, cfg, eng = _engine(name)
    gb = int(g["batch"])
    gold = torch.from_numpy(iv.make_images_int8(cfg, gb, int(g["images_seed"]))).cuda()
    assert np.array_equal(eng.forward(gold).cpu().numpy(), g["logits_int"])
    assert _ln_mlp_blocks(eng, B) == cfg.depth
    imgs = np.concatenate([iv.make_images_int8(cfg, gb, int(g["images_seed"])), iv.make_images_int8(cfg, 4, seed=29)])[:B]
    d = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    names = []
    orig = eng.h.call
    eng.h.call = lambda nm, *a: (names.append(nm), orig(nm, *a))[1]
    try:
        assert eng.fuse_ln_mlp_lockstep is False
        off = eng.forward_ops(d).cpu().numpy()
        assert NAME not in names and names.count("ivit_mlp_fused_planned") == cfg.depth
        del names[:]
        eng.fuse_ln_mlp_lockstep = True
        on = eng.forward_ops(d).cpu().numpy()
        assert names.count(NAME) == cfg.depth and "ivit_mlp_fused_planned" not in names
        # the LayerNorm launches left: the final norm, and norm1 of the blocks whose qkv launch does not carry it
        assert names.count("ivit_layernorm_requant") == 1 + cfg.depth - names.count("ivit_layernorm_linear_i8_qkv_planned")
    finally:
        eng.h.call = orig
        eng.fuse_ln_mlp_lockstep = False
    n = min(B, gb)
    assert np.array_equal(off[:n], g["logits_int"][:n])
    assert np.array_equal(on, off), int((on != off).any(axis=1).sum())
    got = eng.forward(d, nslices=ns).cpu().numpy()
    assert np.array_equal(got, off), int((got != off).any(axis=1).sum())
    replay = eng.capture(d, nstreams=ns)
    for _ in range(2):
        assert np.array_equal(replay().cpu().numpy(), off), "graph replay"
