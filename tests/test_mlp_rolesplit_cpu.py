"""The CPU side of tests/test_mlp_rolesplit_gpu.py: its schedule table is what the host restatement of the dispatch rule gives, and the
oracle alone reaches the conditions that keep the GPU comparison from being vacuous (both ends of norm2's 8-bit range and of the hidden
range, outputs spread over the 16-bit range) at every listed case."""
import pytest

import test_mlp_rolesplit_gpu as rs


@pytest.mark.parametrize("M,cus,balanced,units", rs.SCHEDULES)
def test_schedule_table(M, cus, balanced, units):
    by_default = rs.check_schedule(M, cus, balanced, units)
    rows = [min(16, M - 16 * t) for t in range((M + 15) // 16)]
    print(f"M {M} share {cus}: {'balanced' if balanced else 'round-robin'} {units}, last tile {rows[-1]} rows, role-split by default {by_default}")
    assert all(1 <= n <= rs.TT for wg in units for n in wg) and (balanced or all(n < rs.TT for wg in units for n in wg))


def test_table_reaches_what_it_says():
    """two, three, four and five units per workgroup; 4- and 5-tile bodies; a 4-tile unit followed by a 5-tile one; a last unit of
    one row; workgroups of unlike unit counts in one grid; both schedules"""
    t = {(M, cus): (bal, units) for M, cus, bal, units in rs.SCHEDULES}
    per_wg = {len(wg) for _, units in t.values() for wg in units}
    assert {1, 2, 3, 4, 5} <= per_wg
    assert {bal for bal, _ in t.values()} == {True, False}
    assert any(wg[i:i + 2] == [4, 5] for _, units in t.values() for wg in units for i in range(len(wg)))
    assert t[(321, 2)][1][-1][-1] == 1 and 321 % 16 == 1          # one tile holding one row
    assert 641 % 16 == 1 and 81 % 16 == 1 and 250 % 16 == 10
    assert len({len(wg) for wg in t[(600, 7)][1]}) == 2 and len({len(wg) for wg in t[(641, 2)][1]}) == 2
    assert all(key in t for key in rs.WIDE_LN)


@pytest.mark.parametrize("M,wide_ln", [(s[0], False) for s in rs.SCHEDULES] + [(M, True) for M, _ in rs.WIDE_LN])
def test_oracle_side_is_not_vacuous(M, wide_ln):
    a, h, o = rs.reference(M, wide_ln)
    assert a.shape == (M, rs.C) and h.shape == (M, 4 * rs.C) and o.shape == (M, rs.C)
    rs.check_not_vacuous(M, a, h, o)
