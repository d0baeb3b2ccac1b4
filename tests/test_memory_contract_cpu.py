"""The memory contract of the C-ABI on the CPU twin (oracle/ivit_twin.c), which half of the GPU suite trusts as its reference: every
twinned entry point of tests/abi_cases.py::_cases runs with each array inside its own [1 MiB guard | payload | 1 MiB guard] numpy
arena and must (1) write nothing outside its outputs, (2) give the same bytes whatever lies around its inputs, (3) give the bytes of
the same call on plain arrays.  The harness itself is tested with two planted entries that break rules 1 and 2."""
import ctypes

import numpy as np
import pytest

import abi_cases as A


@pytest.fixture(scope="module")
def twin():
    return A.load_twin()


twin_cases = A.twin_table       # the table, built once per variant and left unchanged (the arenas copy from it)
NAMES = sorted(A.table_names()[0])


def test_every_entry_point_is_in_a_table_or_excluded():
    """a new entry point fails here until someone adds a case for it"""
    missing, stale = A.uncovered_entry_points()
    assert not missing, f"entry points without a case in tests/abi_cases.py: {missing}"
    assert not stale, f"exclusions that name no entry point, or one that has a case: {stale}"


def test_alignment_table_covers_every_entry_with_arrays():
    """check 4 of the device tests reads abi_cases.ALIGN: an entry that gains a case with array arguments but no record there (or in
    TABLES_ONLY) would skip it silently; and every record names array arguments of every case of its entry"""
    missing, wrong = A.alignment_table_gaps()
    assert not missing, f"entries with array arguments and no record in abi_cases.ALIGN: {missing}"
    assert not wrong, f"records of abi_cases.ALIGN that name no array argument: {wrong}"


# input arrays that are functions of a case's scalars alone and so hold the same values whatever the seed: entry -> argument indices
# (the per-tensor dyadics of the requant entries, the Shiftmax tables of one softmax scale)
SEED_FREE_INPUTS = {"requant_i32": {1, 4}, "requant_i16": {1}, "window_attention_fused_lut": {5, 6, 7}, "shiftmax_rowtable": {0, 1, 2}}


def test_tables_from_two_seeds_agree_in_everything_but_contents():
    """tests/test_stream_graph_contract_gpu.py replays a graph captured on one table's arrays on the arrays of the table built from
    abi_cases.SECOND_SEED: the two tables must hold the same entries in the same order with the same scalars, dyadics, host arrays,
    handles, shapes, dtypes and pads, and differ in the contents of their input arrays alone — a case with an rng-drawn scalar fails
    here, not obscurely on the device.  Every input array differs between the seeds unless SEED_FREE_INPUTS names it."""
    pairs = []
    for variant in (0, 1):
        a, b = A.twin_table(variant), A.twin_table(variant, A.SECOND_SEED)
        assert [n for n, _ in a] == [n for n, _ in b]
        pairs += [(n, x, y) for (n, x), (_, y) in zip(a, b)]
    a, b = A.hip_table(None), A.hip_table(None, A.SECOND_SEED)
    assert [(n, s is None, s is not None and s.plans) for n, _, s in a] == [(n, s is None, s is not None and s.plans) for n, _, s in b]
    pairs += [(n, x, y) for (n, x, _), (_, y, _) in zip(a, b)]
    assert pairs
    changed = 0
    for n, x, y in pairs:
        diffs, differ, same = A.table_differences(x, y)
        assert not diffs, (n, diffs)
        assert set(same) <= SEED_FREE_INPUTS.get(n, set()), (n, "input arrays that do not depend on the seed", same)
        changed += len(differ)
    assert changed >= len(pairs)


def test_glds_256_row_tile_is_unreachable():
    """gemm_glds_kernel has a 256-row instantiation that no call can select, which is why the tables hold no case for it: launch_gemm2
    estimates ceil(tiles / slots) * rows with 2 slots per CU for 256-row tiles and, at G2_NSTAGE128 == 2, 4 per CU for 128-row tiles;
    128-row tiles are at most twice as many, so they never need more rounds, and at half the rows per round they always cost less
    (ties go to 256 rows, and there are none).  The rule is restated from csrc/ivit_hip.hip and searched over M, the column tiles and
    CU counts; if the constant or the rule changes this fails, and the tables then need cases on the 256-row side."""
    import os
    import re
    from conftest import ROOT
    csrc = os.path.join(ROOT, "i-vit_amd", "csrc")
    assert re.search(r"#define G2_NSTAGE128 2\b", open(os.path.join(csrc, "ivit_gemm2.h")).read())
    hip = open(os.path.join(csrc, "ivit_hip.hip")).read()
    assert "s256 = 2LL * h->num_cu, s128 = (G2_NSTAGE128 == 2 ? 4LL : 3LL) * h->num_cu;" in hip
    assert "c256 = ((t256 + s256 - 1) / s256) * 256, c128 = ((t128 + s128 - 1) / s128) * 128;" in hip
    assert "if (c128 < c256) gemm_glds_kernel<EPI, 128>" in hip
    M = np.arange(1, 1 << 20, dtype=np.int64)
    for cus in (1, 64, 256, 304):
        for tiles_n in range(1, 13):
            t256, t128 = (M + 255) // 256 * tiles_n, (M + 127) // 128 * tiles_n
            c256, c128 = (t256 + 2 * cus - 1) // (2 * cus) * 256, (t128 + 4 * cus - 1) // (4 * cus) * 128
            assert (c128 < c256).all(), (cus, tiles_n)


@pytest.mark.parametrize("name", NAMES)
def test_twin_memory_contract(twin, name):
    mem = A.NumpyMem()
    fn = getattr(twin, "ivit_cpu_" + name)
    ran = 0
    for variant in (0, 1):
        for i, (n, args) in enumerate(twin_cases(variant)):
            if n != name:
                continue
            what = f"ivit_cpu_{name} (variant {variant}, case {i})"
            got = A.check_contract(fn, None, args, mem, what=what)
            want = A.plain_outputs(fn, None, args, mem)
            for j, (g, w) in enumerate(zip(got, want)):
                assert np.array_equal(g, w), (what, j, int((g != w).sum()))
            ran += 1
    assert ran


# ---------------------------------------------------------------- the harness on two planted bugs
def _view(ptr, n, dtype, offset=0):
    """n elements at ptr + offset elements, as the entry itself would address them"""
    dt = np.dtype(dtype)
    raw = (ctypes.c_uint8 * (n * dt.itemsize)).from_address(ptr.value + offset * dt.itemsize)
    return np.frombuffer(raw, dt)


def _good(h, x, out, n):
    _view(out, n, np.int16)[:] = _view(x, n, np.int16) + 1
    return 0


def _writes_in_front(h, x, out, n):
    _good(h, x, out, n)
    _view(out, 1, np.int16, offset=-1)[:] = 7                 # one element in front of its output
    return 0


def _reads_behind(h, x, out, n):
    _good(h, x, out, n)
    _view(out, 1, np.int16)[:] += _view(x, 1, np.int8, offset=2 * n).astype(np.int16)     # the byte behind its input
    return 0


def _skips_last(h, x, out, n):
    _view(out, n - 1, np.int16)[:] = _view(x, n - 1, np.int16) + 1
    return 0


def test_harness_catches_planted_bugs():
    """check 1 fails on the entry that writes in front of its output and check 2 on the one that reads behind its input, each with its
    own message, and neither on the other; an entry that leaves an output element unwritten is caught too; the sound entry passes"""
    mem = A.NumpyMem()
    x = np.arange(-500, 500, dtype=np.int16)
    args = [("in", x), ("out", np.zeros(1000, np.int16)), 1000]
    want = (x + 1).view(np.uint8)
    assert np.array_equal(A.check_contract(_good, None, args, mem)[0], want)
    assert np.array_equal(A.plain_outputs(_good, None, args, mem)[0], want)
    with pytest.raises(A.ContractError, match="2 bytes written IN FRONT of the output"):
        A.check_contract(_writes_in_front, None, args, mem)
    with pytest.raises(A.ContractError, match="depend on what lies around the inputs"):
        A.check_contract(_reads_behind, None, args, mem)
    with pytest.raises(A.ContractError, match="2 bytes of the output never written"):
        A.check_contract(_skips_last, None, args, mem)
    # pad columns: an input's are filled like the guards, an output's must keep the fill
    xp = np.zeros((4, 8), np.int16)
    xp[:, :5] = 3

    def rowsum(h, x, out, rows, n, ld):
        _view(out, rows, np.int16)[:] = _view(x, rows * ld, np.int16).reshape(rows, ld)[:, :n].sum(axis=1)
        return 0

    def rowsum_unmasked(h, x, out, rows, n, ld):
        _view(out, rows, np.int16)[:] = _view(x, rows * ld, np.int16).reshape(rows, ld).sum(axis=1)
        return 0
    pargs = [("in", xp, 5), ("out", np.zeros(4, np.int16)), 4, 5, 8]
    assert np.array_equal(A.check_contract(rowsum, None, pargs, mem)[0].view(np.int16), np.full(4, 15, np.int16))
    with pytest.raises(A.ContractError, match="depend on what lies around the inputs"):
        A.check_contract(rowsum_unmasked, None, pargs, mem)
    zargs = [("in", xp, ("zero", 5)), ("out", np.zeros(4, np.int16)), 4, 5, 8]      # a pad the header demands to be zero stays zero
    assert np.array_equal(A.check_contract(rowsum_unmasked, None, zargs, mem)[0].view(np.int16), np.full(4, 15, np.int16))


# ---------------------------------------------------------------- overlapping arguments: the table, the header, the harness
def test_overlap_table_is_consistent():
    """every record of abi_cases.INPLACE names an entry with cases, an activation input and an output that are arrays of equal size in
    every case of it, and carries its reason; the two entries refused by decree are not in it"""
    assert not A.overlap_table_gaps(), A.overlap_table_gaps()
    for name in A.ALWAYS_REFUSED:
        assert name not in A.INPLACE and name in A.ALIGN


def _header_comment_in_front_of(hdr, name):
    """the text between the end of the previous declaration and the prototype of ivit_<name>"""
    import re
    m = re.search(r"\bint ivit_%s\(" % re.escape(name), hdr)
    assert m, name
    return hdr[hdr.rfind(";", 0, m.start()) + 1:m.start()]


def test_header_has_an_overlap_line_for_every_entry_with_arrays():
    """include/ivit.h states the contract once and has an "Overlap:" line in front of every entry with an ALIGN record; the line speaks
    of an in-place form, and names both arguments of the pair, exactly where abi_cases.INPLACE has a record; the entries whose kernels
    declare their pointers __restrict__ are not among them"""
    import os
    import re
    from conftest import ROOT
    from ivit_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ivit.h")).read()
    assert "overlapping arguments:" in hdr[:hdr.index("#ifndef IVIT_H")]
    # (the two ragged front-end entries are in no table: tests/test_pil_resize_gpu.py runs them)
    for name in sorted(A.ALIGN) + ["resize_center_crop_u8_pil", "eval_transform_u8"]:
        lines = re.findall(r"\bOverlap:.*?\*/", _header_comment_in_front_of(hdr, name), re.S)     # a comment of its own, or the end of the entry's
        assert len(lines) == 1, (name, lines)
        assert ("in place" in lines[0]) == (name in A.INPLACE), (name, lines[0])
        params = _lib.ABI.functions["ivit_" + name].params
        for i, o in A.INPLACE.get(name, {}):
            assert re.search(r"\b%s == %s\b" % (params[i + 1].name, params[o + 1].name), lines[0]), (name, lines[0])
    assert "IVIT_VERSION 111" in hdr
    assert not {"requant_i16", "shiftgelu_requant", "shiftgelu_requant_lut"} & set(A.INPLACE)


class _FakeHandle:
    """what check_overlap asks of a handle, for entries written in Python: .h, and .lib.ivit_last_error(h)"""
    def __init__(self):
        self.h, self.lib, self.err = None, self, b""

    def ivit_last_error(self, h):
        return self.err


def _planted(F, extent_of_x=lambda n: 2 * n, refuses=True, sequential=False):
    """out[i] = x[i] + 1 over n int16 values; sequential: out[i] = x[i] + x[(i + 1) % n] (mod 2^16), one element at a time from the last
    to the first, so that in place x[i + 1] already holds out[i + 1].  Refuses an `out` that overlaps [x, x + extent_of_x(n)) unless it
    is x itself"""
    def entry(h, x, out, n):
        lo, hi = x.value, x.value + extent_of_x(n)
        if refuses and out.value != x.value and out.value < hi and lo < out.value + 2 * n:
            F.err = b"planted: x and out overlap"
            return 1
        xs, os_ = _view(x, n, np.int16), _view(out, n, np.int16)
        if not sequential:
            os_[:] = xs + 1
            return 0
        first = int(xs[0])
        for i in range(n - 1, -1, -1):
            os_.view(np.uint16)[i] = (int(xs[i]) + (int(xs[i + 1]) if i + 1 < n else first)) & 0xFFFF
        return 0
    return entry


def test_overlap_harness_catches_planted_entries():
    """check_overlap on four entries written in Python: the sound one (refuses overlaps, elementwise in place) passes; one that does
    not refuse, one declared in place whose result depends on the order of its loads and stores, and one that over-estimates the
    extent of its input (and so refuses arrays that merely touch) are each caught with their own message"""
    mem, F = A.NumpyMem(), _FakeHandle()
    n = 640                     # 1280 bytes, a multiple of 256: the adjacent placements touch, so two bytes too many are seen
    x = np.arange(-320, 320, dtype=np.int16)
    args = [("in", x), ("out", np.zeros(n, np.int16)), n]
    kw = dict(inputs=(0,), inplace={(0, 1): "elementwise"})
    A.check_overlap(_planted(F), F, args, mem, None, "sound", **kw)
    with pytest.raises(A.ContractError, match="not refused"):
        A.check_overlap(_planted(F, refuses=False), F, args, mem, None, "never refuses", inputs=(0,), inplace={})
    with pytest.raises(A.ContractError, match="same start, run 1: argument 1: .* bytes differ from the call on disjoint arrays"):
        A.check_overlap(_planted(F, sequential=True), F, args, mem, None, "order-dependent", **kw)
    with pytest.raises(A.ContractError, match="b behind a: status 1, expected IVIT_OK: planted: x and out overlap"):
        A.check_overlap(_planted(F, extent_of_x=lambda n: 2 * n + 2), F, args, mem, None, "over-estimated extent", **kw)
    # a pair that is NOT declared in place is refused at the same start too: the sound entry, asked without its record, is caught
    with pytest.raises(A.ContractError, match="same start: status 0, expected IVIT_ERR_INVALID"):
        A.check_overlap(_planted(F), F, args, mem, None, "undeclared", inputs=(0,), inplace={})
