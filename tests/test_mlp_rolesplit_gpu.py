"""The role-split fused Mlp (mlp384rs_kernel of csrc/ivit_mlp_rs.h), with and without its LayerNorm head, against the CPU ORACLE's
operators at every unit schedule its hand-over counters F_H / F_G / F_R / F_A / F_D go through: two to five units per workgroup, 4- and
5-tile unit bodies, the switch from two to three 32-token tiles inside one workgroup, a last unit of one row, balanced and round-robin.
A few hundred rows on a share of 1, 2 or 7 CUs (ivit_set_cu_share) reach them.  ivit_mlp_fused_planned is given the oracle's own norm2
rows, and the scratch8 of ivit_layernorm_mlp_fused_planned is compared with the oracle's norm2 rows too, never with another HIP
kernel's.  Bit-exact, every row, three launches each into freshly poisoned buffers with a canary row behind the last one.
tests/test_mlp_rolesplit_cpu.py checks the table below and the oracle's side of it without a GPU."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from ivit_amd import _lib  # noqa: E402
from test_ln_mlp_lockstep_gpu import Case, P, dyv, S_IN, POISON  # noqa: E402

_P = ctypes.c_void_p
C = 384
TT = 5                      # Mlp384Geo::TT: the most 16-row tiles of a unit
POISON8 = 77
LN_NAME = "ivit_layernorm_mlp_fused_planned"

# (M, CU share, balanced, tiles per unit of every workgroup).  Share 0: the whole device, one unit in all
SCHEDULES = [
    (81, 1, False, [[4, 2]]),                                   # smallest two-unit workgroup; the last unit ends in a 1-row tile
    (250, 2, False, [[4, 4], [4, 4]]),                          # two full units each; ragged last tile (10 rows)
    (313, 2, True, [[5, 5], [5, 5]]),                           # the 5-tile body twice
    (205, 1, True, [[4, 4, 5]]),                                # three units; 2 -> 3 32-token tiles inside one workgroup
    (321, 2, False, [[4, 4, 4], [4, 4, 1]]),                    # three units; the last unit is ONE row
    (641, 2, True, [[5, 5, 5, 5], [4, 4, 4, 4, 5]]),            # 4 and 5 units; unlike workgroups; last tile one row
    (600, 7, False, [[4, 4], [4, 4], [4, 2], [4], [4], [4], [4]]),      # workgroups with 1 and 2 units in one grid
    (550, 7, True, [[5]] * 7),                                  # one 5-tile unit per workgroup on the role-split kernel
    (1, 0, False, [[1]]),                                       # one unit of one tile: select 2 only, the LayerNorm entry refuses
    (17, 0, False, [[2]]),                                      # one unit of two tiles: the same
]
WIDE_LN = [(321, 2), (205, 1)]


def schedule(M, cus):
    """Host restatement of csrc/ivit_hip.hip's mlp_fused_launch (grid, balanced or round-robin, which kernel by default) and of
    csrc/ivit_mlp.h's MLP_UNIT_SCHEDULE (the units of every workgroup) at width 384.  cus: the CUs the launch is sized for.
    Returns (balanced, [[tiles of unit 0, of unit 1, ...] per workgroup], role-split by the default rule)."""
    ntiles = (M + 15) // 16
    nunits = (ntiles + TT - 2) // (TT - 1)                  # 64-token units
    grid = min(nunits, cus)
    rounds_fixed, rounds_bal = -(-nunits // grid), -(-ntiles // (TT * grid))
    balanced = rounds_bal < rounds_fixed
    wgs = []
    for b in range(grid):
        t_beg, t_end = ntiles * b // grid, ntiles * (b + 1) // grid
        n_own = t_end - t_beg
        if balanced:
            nu = -(-n_own // TT)
            tile0 = [t_beg + n_own * i // nu for i in range(nu + 1)]
            wgs.append([tile0[i + 1] - tile0[i] for i in range(nu)])
        else:
            nu = (nunits - b + grid - 1) // grid
            tile0 = [min((b + i * grid) * (TT - 1), ntiles) for i in range(nu)]
            wgs.append([min(TT - 1, ntiles - t) for t in tile0])
    assert sum(map(sum, wgs)) == ntiles
    return balanced, wgs, nunits > cus


def check_schedule(M, cus, balanced, units, num_cu=256):
    """the table's row is what the dispatch rule gives; from two units per CU on the default rule takes the role-split kernel too"""
    got = schedule(M, cus if cus else num_cu)
    assert got[:2] == (balanced, units), (M, cus, got)
    assert got[2] == (cus != 0), (M, cus, got)
    return got[2]


@functools.lru_cache(maxsize=None)
def reference(M, wide_ln=False):
    """the host operands and the oracle's (norm2 rows, hidden, out) of a case, computed once and left unchanged"""
    c = Case(None, C, M, seed=9000 + M, wide_ln=wide_ln)
    a, h, o = c.oracle()
    for t in (a, h, o):
        t.setflags(write=False)
    return a, h, o


def check_not_vacuous(M, a, h, o):
    """from 80 rows on both ends of norm2's and of the hidden range are reached and the outputs are spread over the 16-bit range"""
    if M >= 80:
        assert a.min() == -128 and a.max() == 127
        assert h.min() == -128 and h.max() == 127
        assert len(np.unique(o)) > 1000


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


def num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def run_mlp(c, a8, select, want, what):
    """ivit_mlp_fused_planned on the oracle's norm2 rows, the identity branch x16, the plan pinned to `select`"""
    M = c.M
    out = torch.full((M + 1, C), POISON, dtype=torch.int16, device="cuda")
    assert c.H.lib.ivit_mlp_plan_select(c.mp, select) == 0
    try:
        c.H.call("ivit_mlp_fused_planned", c.mp, P(a8), P(c.tab), dyv(c.dm), dyv(c.dr), P(c.d["x16"]), P(out), M)
    finally:
        assert c.H.lib.ivit_mlp_plan_select(c.mp, 0) == 0
    got = out.cpu().numpy()
    assert (got[M] == POISON).all(), (what, "wrote behind the last row")
    assert np.array_equal(got[:M].astype(np.int32), want), (what, int((got[:M] != want).sum()))


def ln_args(c, scratch, out):
    d = c.d
    return (c.mp, P(d["x16"]), float(S_IN), P(d["bias_int"]), P(d["sc"]), P(d["dln"]), P(scratch), P(c.tab), dyv(c.dm), dyv(c.dr), P(out), c.M)


def run_ln(c, a, want, what):
    """ivit_layernorm_mlp_fused_planned: it refuses every kernel but the role-split one, so a return of 0 says which kernel ran.  The
    scratch against the ORACLE's norm2 rows; row M of the scratch and of the output keep their poison."""
    M = c.M
    out = torch.full((M + 1, C), POISON, dtype=torch.int16, device="cuda")
    scratch = torch.full((M + 1, C), POISON8, dtype=torch.int8, device="cuda")
    c.H.call(LN_NAME, *ln_args(c, scratch, out))
    got, s8 = out.cpu().numpy(), scratch.cpu().numpy()
    assert (got[M] == POISON).all() and (s8[M] == POISON8).all(), (what, "wrote behind the last row")
    assert np.array_equal(s8[:M].astype(np.int32), a), (what, "norm2 rows", int((s8[:M] != a).sum()))
    assert np.array_equal(got[:M].astype(np.int32), want), (what, int((got[:M] != want).sum()))


@pytest.mark.parametrize("M,cus,balanced,units", SCHEDULES)
def test_rolesplit_vs_oracle(H, M, cus, balanced, units):
    """Every entry that reaches mlp384rs_kernel, at one row of the schedule table: pinned (select 2) and, where the default rule picks
    it, unpinned, both on the oracle's norm2 rows (mlp384rs_kernel<FMA, 0>); the LayerNorm-headed entry (mlp384rs_kernel<FMA, 1>), or
    its refusal where one unit per workgroup leaves it nothing to overlap."""
    by_default = check_schedule(M, cus, balanced, units, num_cu())
    a, h, o = reference(M)
    check_not_vacuous(M, a, h, o)
    c = Case(H, C, M, seed=9000 + M)
    try:
        a8 = torch.from_numpy(a.astype(np.int8)).cuda()
        H.set_cu_share(cus)
        try:
            for rep in range(3):
                run_mlp(c, a8, 2, o, ("select 2", rep))
                if by_default:
                    run_mlp(c, a8, 0, o, ("select 0", rep))
                    run_ln(c, a, o, ("layernorm head", rep))
            if not by_default:
                out = torch.full((M + 1, C), POISON, dtype=torch.int16, device="cuda")
                scratch = torch.full((M + 1, C), POISON8, dtype=torch.int8, device="cuda")
                assert getattr(H.lib, LN_NAME)(H.h, *ln_args(c, scratch, out)) == _lib.IVIT_ERR_UNSUPPORTED
                assert "role-split" in H.lib.ivit_last_error(H.h).decode()
                torch.cuda.synchronize()
                assert (out == POISON).all() and (scratch == POISON8).all()
        finally:
            H.set_cu_share(0)
    finally:
        c.close()


@pytest.mark.parametrize("M,cus", WIDE_LN)
def test_rolesplit_ln_head_wide_requant(H, M, cus):
    """One LayerNorm channel whose multiplier is out of the two-operation requant's range: the head takes its v_rndne_f64 form
    (ln_stage_constants answers false), at a three-unit workgroup of either schedule."""
    row = next(s for s in SCHEDULES if s[:2] == (M, cus))
    assert check_schedule(*row, num_cu())
    a, h, o = reference(M, True)
    check_not_vacuous(M, a, h, o)
    c = Case(H, C, M, seed=9000 + M, wide_ln=True)
    try:
        H.set_cu_share(cus)
        try:
            for rep in range(3):
                run_ln(c, a, o, ("wide layernorm head", rep))
        finally:
            H.set_cu_share(0)
    finally:
        c.close()
