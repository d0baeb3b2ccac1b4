"""The multiply-then-add requant (the FMA = false instantiations: (double) z * c + magic, the reference's two roundings) in every
kernel that has one, against the CPU oracle's operators, every row, bit for bit.

Two ways to make a plan answer single_fma_ok == 0:
  "neg"     the recipe of tests/test_ws192_gpu.py::layer: channel 5 gets a negative multiplier and a bias of 9.5e6, so that
            |m| zmax >= 2^53 and linear_plan_fma_kernel refuses c <= 0.  Reaches every instantiation, but no operand at which the
            two forms give different integers.
  "triple"  one channel's multiplier row is written as (m, 2^-e) of tests/golden/requant_two_roundings.npz and its bias is set so that
            ONE chosen element's accumulator is the recorded z: there one rounding and two roundings are different integers, and the
            triple is picked so that the output behind the residual QuantAct differs too.  c > 0 and zmax < 2^31: the plan's answer
            is the step proof finding a true counterexample.  8-bit epilogues (fc1's hidden tile, the qkv scatter, plain 8-bit
            rows) take the recorded triples of the 8-bit range, e = 47 .. 49.
Every plan's answer is also compared with a host restatement of the proof that enumerates the differing z of every channel exactly
(tests/two_roundings.py::differing)."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from oracle import oracle as orc  # noqa: E402
import two_roundings as tr  # noqa: E402
from test_ln_mlp_lockstep_gpu import Case, P, dyv, S_IN, S_LN_OUT, S_FC1_OUT, S_FC2_OUT, POISON, NAME as LN_LOCKSTEP  # noqa: E402
from test_ws192_gpu import layer, dev, S_MID, S_FIN, S_RES  # noqa: E402

_P = ctypes.c_void_p
BAD = 5                 # the channel of the "neg" recipe
HIT = 7                 # the channel of the "triple" recipe
POISON8 = 77
LN_ROLESPLIT = "ivit_layernorm_mlp_fused_planned"


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def triples(K):
    """the recorded (z, m, e, two, one) for K = 1536 or 384 (16-bit range), or "bits8" (8-bit range; |z| > 10^7: the bias carries it)"""
    return [tuple(r) for r in load_golden("requant_two_roundings.npz")[K if K == "bits8" else f"k{K}"].tolist()]


def query(H, p):
    a, b = ctypes.c_int(-1), ctypes.c_int(-1)
    assert H.lib.ivit_linear_plan_query(p, ctypes.byref(a), ctypes.byref(b)) == 0
    return a.value, b.value


def expect_flags(w, b, table):
    """Host restatement of linear_plan_kernel and linear_plan_fma_kernel (csrc/ivit_hip.hip): (pipelined_ok, single_fma_ok) of a layer
    with weights w [N, K], bias b and multiplier table [N, 2] of (m, 2^-e).  The step proof's answer is computed another way: it
    succeeds exactly when no z within the channel's bound rounds differently once and twice inside the 16-bit range."""
    zmax = 128 * np.abs(w.astype(np.int64)).sum(axis=1) + np.abs(b.astype(np.int64))
    m, r = table[:, 0], table[:, 1]
    pipelined = int((np.abs(m * r) * zmax < 2147483000.0).all())
    unproven = np.nonzero(~(np.abs(m) * zmax < 9007199254740992.0))[0]          # the cheap bound fails: the step proof decides
    if not pipelined:
        return 0, int(unproven.size == 0)
    for n in unproven:
        if not m[n] * r[n] > 0 or not zmax[n] < 2147483000 or tr.differing(int(m[n]), int(round(-np.log2(r[n]))), int(zmax[n]), lim=32768):
            return 1, 0
    return 1, 1


def pick_triple(K, identity, start):
    """the first recorded triple from number `start` on (the cases rotate through both signs of z) whose two results are different
    integers BEHIND the residual QuantAct with this identity value too"""
    for z, m, e, two, one in triples(K)[start % 8:] + triples(K)[:start % 8]:
        fin = [int(Case.residual_act(np.array([[t]]), np.array([[identity]], np.int16))[0, 0]) for t in (two, one)]
        if fin[0] != fin[1]:
            return z, m, e, two, one, fin[0], fin[1]
    raise AssertionError("no recorded triple survives the residual QuantAct")


# ---------------------------------------------------------------- the fused Mlp kernels
def neg_layer(which):
    def tweak(c):
        s, b = (c.s1, c.b1) if which == 1 else (c.s2, c.b2)
        s[BAD] = -s[BAD]
        b[BAD] = 9500000
        c.hit = None
    return tweak


def triple_fc2(c):
    """fc2's channel HIT of row M // 2 lands on a recorded z (K = 1536 triples at width 384; the K = 384 ones fit fc2 of the narrower
    widths: |z| <= 128 * 127 * 384 is inside every accumulator range)"""
    row = c.M // 2
    z, m, e, two, one, fin2, fin1 = pick_triple(1536 if c.C == 384 else 384, c.x16[row, HIT], c.M)
    c.b2[HIT] += z - int(c.chain()["acc2"][row, HIT])
    c.rows2[HIT] = (m, e)
    c.hit = (row, z, two, one, fin2, fin1)


def triple_fc1(c):
    """fc1's channel HIT of row M // 2 lands on a recorded z of the 8-bit range: the HIDDEN byte differs between one rounding and two.
    The triple is the first (from number M on) at which that byte changes the row's output behind ShiftGELU, fc2 and both QuantActs."""
    row, t8 = c.M // 2, triples("bits8")
    a8 = c.chain()["a"].astype(np.int8)
    bias0 = int(c.b1[HIT])
    acc = int(orc.linear_i8(a8[row:row + 1], c.w1, c.b1)[0, HIT])
    c.hit = None
    for z, m, e, two, one in t8[c.M % len(t8):] + t8[:c.M % len(t8)]:
        c.b1[HIT] = bias0 + z - acc
        c.rows1[HIT] = (m, e)
        h = c.chain()["h"][row:row + 1]
        assert h[0, HIT] == two != one
        h1 = h.copy()
        h1[0, HIT] = one
        o2, o1 = (c.from_hidden(hh, c.x16[row:row + 1])["o"][0] for hh in (h, h1))
        if (o2 != o1).any():
            c.hit8 = (row, z, two, one, int((o2 != o1).sum()))
            return
    raise AssertionError("no recorded 8-bit triple changes the output row")


TWEAKS = {"fc1 neg": neg_layer(1), "fc2 neg": neg_layer(2), "fc2 triple": triple_fc2, "fc1 triple": triple_fc1}
ENTRIES = {384: ("lockstep", "rolesplit", "ln rolesplit", "ln lockstep"), 192: ("lockstep", "ln lockstep"), 256: ("lockstep",)}


def run_entry(c, entry, a, a8, want):
    """one launch of an Mlp entry into a poisoned output with a canary row; every row against the oracle"""
    H, M = c.H, c.M
    out = torch.full((M + 1, c.C), POISON, dtype=torch.int16, device="cuda")
    if entry in ("lockstep", "rolesplit"):          # mlp384_kernel / mlp192_kernel / mlp256_kernel | mlp384rs_kernel<., 0>
        assert H.lib.ivit_mlp_plan_select(c.mp, 1 if entry == "lockstep" else 2) == 0
        try:
            H.call("ivit_mlp_fused_planned", c.mp, P(a8), P(c.tab), dyv(c.dm), dyv(c.dr), P(c.d["x16"]), P(out), M)
        finally:
            assert H.lib.ivit_mlp_plan_select(c.mp, 0) == 0
    elif entry == "ln rolesplit":                   # mlp384rs_kernel<., 1>: refuses any other kernel
        d = c.d
        scratch = torch.full((M + 1, c.C), POISON8, dtype=torch.int8, device="cuda")
        H.call(LN_ROLESPLIT, c.mp, P(d["x16"]), float(S_IN), P(d["bias_int"]), P(d["sc"]), P(d["dln"]), P(scratch), P(c.tab), dyv(c.dm),
               dyv(c.dr), P(out), M)
        s8 = scratch.cpu().numpy()
        assert (s8[M] == POISON8).all() and np.array_equal(s8[:M].astype(np.int32), a), entry
    else:                                           # mlp384ln_kernel / mlp192ln_kernel
        H.call(LN_LOCKSTEP, *c.args(out))
    got = out.cpu().numpy()
    assert (got[M] == POISON).all(), (entry, "wrote behind the last row")
    bad = int((got[:M] != want).sum())
    if c.hit:
        print(f"    {entry}: element {int(got[c.hit[0], HIT])} (two roundings {c.hit[4]}, one {c.hit[5]}), mismatches {bad}")
    assert bad == 0, (entry, bad)


@pytest.mark.parametrize("kind", sorted(TWEAKS))
@pytest.mark.parametrize("C,M,cus", [(384, 321, 2), (384, 205, 1), (192, 197, 0), (192, 1123, 1), (256, 197, 0), (256, 1000, 0)])
def test_mlp_two_rounding_form_vs_oracle(H, C, M, cus, kind):
    """width 384: mlp384_kernel<false>, mlp384rs_kernel<false, 0>, mlp384rs_kernel<false, 1>, mlp384ln_kernel<false> at a three-unit
    workgroup of either schedule; width 192: mlp192_kernel<false>, mlp192ln_kernel<false>; width 256: mlp256_kernel<false>"""
    c = Case(H, C, M, seed=5000 + 7 * C + M, tweak=TWEAKS[kind])
    try:
        f1 = query(H, c.p1)
        f2 = query(H, c.p2)
        e1 = expect_flags(c.w1, c.b1, Case.table(iv.freeze.dyadic(c.s1, S_FC1_OUT), c.rows1))
        e2 = expect_flags(c.w2, c.b2, Case.table(iv.freeze.dyadic(c.s2, S_FC2_OUT), c.rows2))
        print(f"C {C} M {M} share {cus} {kind}: fc1 (pipelined_ok, single_fma_ok) {f1} expected {e1}, fc2 {f2} expected {e2}")
        assert f1 == e1 and f2 == e2
        assert (f1 if kind.startswith("fc1") else f2) == (1, 0) and (f2 if kind.startswith("fc1") else f1) == (1, 1)
        ch = c.chain()
        if kind == "fc1 triple":
            row, z, two, one, nout = c.hit8
            assert ch["h"][row, HIT] == two != one
            print(f"    hidden element: two roundings {two}, one {one}; {nout} outputs of row {row} depend on it")
        if c.hit:
            row, z, two, one, fin2, fin1 = c.hit
            assert ch["acc2"][row, HIT] == z and ch["t"][row, HIT] == two != one and ch["o"][row, HIT] == fin2 != fin1
        a8 = torch.from_numpy(ch["a"].astype(np.int8)).cuda()
        H.set_cu_share(cus)
        try:
            for entry in ENTRIES[C]:
                run_entry(c, entry, ch["a"], a8, ch["o"])
        finally:
            H.set_cu_share(0)
    finally:
        c.close()


# ---------------------------------------------------------------- single layers: gemm_ws_qkv_kernel at K = 384, the persistent kernels
@functools.lru_cache(maxsize=None)
def ln_rows(M):
    """16-bit rows, LayerNorm constants and the oracle's norm1 + qact of them at width 384: the operands of tests/test_ln_mlp_lockstep_gpu.py"""
    c = Case(None, 384, M, seed=6000 + M)
    return c, c.chain()["a"].astype(np.int8)


@functools.lru_cache(maxsize=None)
def lin_case(M, N, K, bits, kind):
    """layer(N, bits, ., K) of tests/test_ws192_gpu.py on 8-bit rows (norm1's at K = 384, uniform at K = 1536); "triple": channel HIT's
    multiplier row and bias rewritten so that row M // 2 lands on a recorded z.  The oracle's requant t, and behind the residual
    QuantAct o with 16-bit identity rows over the whole range."""
    rng = np.random.default_rng(M + N + K)
    w, b, s_pre, s_out = layer(N, bits, kind != "neg", K)
    x = ln_rows(M)[1] if K == 384 else rng.integers(-128, 128, (M, K), dtype=np.int8)
    res = rng.integers(-32768, 32768, (M, N)).astype(np.int16)
    res[0, 0::2], res[0, 1::2] = 32767, -32768
    table, otable, b, hit = iv.freeze.dyadic(s_pre, s_out), orc.dyadic(s_pre, s_out), b.copy(), None
    plain = expect_flags(w, b, table)
    if kind == "triple":
        row = M // 2
        res[row, HIT] = 1234
        if bits == 16:
            z, m, e, two, one, fin2, fin1 = pick_triple(K, res[row, HIT], M // 100 + N // 384)
        else:
            t8 = triples("bits8")
            z, m, e, two, one = t8[(M // 100 + N // 384) % len(t8)]
            fin2 = fin1 = None
        b[HIT] += z - int(orc.linear_i8(x, w, b)[row, HIT])
        Case.table(table, {HIT: (m, e)})
        Case.table(otable, {HIT: (m, e)})
        hit = (row, z, two, one, fin2, fin1)
    acc = orc.linear_i8(x, w, b)
    t = orc.requant(acc, otable, bits)
    o = orc.requant(t, orc.dyadic(S_MID, S_FIN), 16, res.astype(np.int32), orc.dyadic(S_RES, S_FIN)) if bits == 16 else None
    if hit:
        assert acc[row, HIT] == z and t[row, HIT] == two != one and (bits == 8 or o[row, HIT] == fin2 != fin1)
        assert plain == (1, 1)          # without the triple the layer takes the one-FMA form: the triple alone decides
    return dict(x=x, w=w, b=b, table=table, t=t, o=o, res=res, hit=hit, flags=expect_flags(w, b, table))


class Layer:
    """device copies of a lin_case and its plan, prepared for gemm_ws_qkv_kernel or left as created; the plan's answer is checked"""

    def __init__(self, H, case, prepare):
        self.keep = [dev(case[k]) for k in ("w", "b", "table")]
        N, K = case["w"].shape
        self.plan = H.linear_plan(P(self.keep[0]), P(self.keep[1]), P(self.keep[2]), N, K)
        if prepare:
            H.call("ivit_linear_plan_prepare_ws", self.plan.p)
        got = (int(self.plan.pipelined_ok), int(self.plan.single_fma_ok))
        print(f"    plan {N} x {K}: (pipelined_ok, single_fma_ok) {got} expected {case['flags']}")
        assert got == case["flags"] == (1, 0)
        self.p = self.plan.p

    def close(self):
        self.plan.close()


def check_rows(out, want, M, what, hit=None):
    got = out.cpu().numpy()
    assert (got[M:] == (POISON8 if got.dtype == np.int8 else POISON)).all(), (what, "wrote behind the last row")
    bad = int((got[:M] != want).sum())
    if hit:
        print(f"    {what}: element {int(got[hit[0], HIT])}, mismatches {bad}")
    assert bad == 0, (what, bad)


def poisoned(rows, cols, bits):
    return torch.full((rows, cols), POISON8 if bits == 8 else POISON, dtype=torch.int8 if bits == 8 else torch.int16, device="cuda")


def run_residual(H, pl, case, M, what):
    out = poisoned(M + 1, case["w"].shape[0], 16)
    dm, dr = iv.freeze.dyadic(S_MID, S_FIN), iv.freeze.dyadic(S_RES, S_FIN)
    xd, rd = dev(case["x"]), dev(case["res"])
    H.call("ivit_linear_i8_requant_residual_planned", pl.p, P(xd), dyv(dm), dyv(dr), P(rd), P(out), M)
    check_rows(out, case["o"], M, what, case["hit"])


@pytest.mark.parametrize("cus", [0, 2])
def test_ws384_two_rounding_form_vs_oracle(H, cus):
    """gemm_ws_qkv_kernel<Ws384Geo, false, LN, EPI> on prepared plans, 3 x 197 = 591 tokens (19 tiles of 32; on a share of two CUs two
    workgroups of 9 and 10): LN on and off with the qkv scatter and with the plain 8-bit rows, and proj + residual (LN off) by both
    recipes.  The same residual call on the plan as created runs the launch-per-tile kernel."""
    B, T, HH, DH, K = 3, 197, 6, 64, 384
    M = B * T
    lc, a8 = ln_rows(M)
    keep = [dev(t) for t in (lc.x16, lc.bias_int, lc.sc, iv.freeze.dyadic(lc.s_pre, S_LN_OUT))]
    ln = (P(keep[0]), float(S_IN), P(keep[1]), P(keep[2]), P(keep[3]))
    xd = dev(a8)
    res = [(kind, lin_case(M, K, K, 16, kind)) for kind in ("neg", "triple")]
    H.set_cu_share(cus)
    try:
        for kind in ("neg", "triple"):
            qc = lin_case(M, 3 * K, K, 8, kind)
            want_qkv = qc["t"].reshape(B, T, 3, HH, DH).transpose(2, 0, 3, 1, 4).reshape(3, B * HH * T, DH)
            assert qc["t"].min() == -128 and qc["t"].max() == 127 and len(np.unique(qc["t"])) > 100
            pq = Layer(H, qc, True)
            for form in ("ln", "alone"):
                q, k, v = (poisoned(B * HH * T + 1, DH, 8) for _ in range(3))
                if form == "ln":
                    H.call("ivit_layernorm_linear_i8_qkv_planned", pq.p, *ln, P(q), P(k), P(v), B, T, HH, DH)
                else:
                    H.call("ivit_linear_i8_qkv_planned", pq.p, P(xd), P(q), P(k), P(v), B, T, HH, DH, 0)
                for i, t in enumerate((q, k, v)):
                    check_rows(t, want_qkv[i], B * HH * T, ("qkv scatter", kind, form, "qkv"[i]))
                out = poisoned(M + 1, 3 * K, 8)
                if form == "ln":
                    H.call("ivit_layernorm_linear_i8_requant_planned", pq.p, *ln, P(out), M)
                else:
                    H.call("ivit_linear_i8_requant_planned", pq.p, P(xd), 8, P(out), M)
                check_rows(out, qc["t"], M, ("plain 8-bit rows", kind, form), qc["hit"])
            pq.close()
        for kind, rc in res:
            assert rc["o"].min() == -32768 and rc["o"].max() == 32767
            for prepare in (True, False):
                pl = Layer(H, rc, prepare)
                run_residual(H, pl, rc, M, ("proj + residual", kind, "prepared" if prepare else "as created"))
                pl.close()
    finally:
        H.set_cu_share(0)


@pytest.mark.parametrize("M", [300, 200, 100])
@pytest.mark.parametrize("N,K", [(1536, 384), (384, 1536)])
def test_persistent_gemm_two_rounding_form_vs_oracle(H, M, N, K):
    """ivit_linear_i8_requant_planned (8 and 16 bit) and ivit_linear_i8_requant_residual_planned on plans as created: M = 300 runs
    gemm_as_kernel<EPI, ., false> (K = 384 n, M >= 256), M = 200 gemm_ps_kernel<EPI, false> (M >= 128), M = 100 the launch-per-tile
    kernels; the residual epilogue is on the persistent kernels at N >= 512 only.  Both recipes at 8 and 16 bit and behind the
    residual: fc1's shape with K = 384 triples, fc2's with K = 1536 triples, 8 bit with the 8-bit-range triples."""
    for bits, kind in ((8, "neg"), (8, "triple"), (16, "neg"), (16, "triple")):
        c = lin_case(M, N, K, bits, kind)
        pl = Layer(H, c, False)
        try:
            out, xd = poisoned(M + 1, N, bits), dev(c["x"])
            H.call("ivit_linear_i8_requant_planned", pl.p, P(xd), bits, P(out), M)
            check_rows(out, c["t"], M, ("requant", bits, kind), c["hit"])
            if bits == 16:
                run_residual(H, pl, c, M, ("requant + residual", kind))
        finally:
            pl.close()
