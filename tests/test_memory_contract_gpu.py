"""The memory contract of the C-ABI on the device: every entry point writes only its outputs and reads only its inputs.

Operators: every case of both tables of tests/abi_cases.py runs with each array inside its own [1 MiB guard | payload | 1 MiB guard]
device arena and must (1) leave both guards of every output and the bytes it documents as not written untouched, under two fills,
and write every other byte; (2) give the same bytes when the surroundings of its inputs (guards and pad columns) change from 0x7F
to 0xFF; (3) give the bytes of the same call on plain allocations, and of the CPU twin where it has one; (4) behave as
abi_cases.ALIGN records when one activation pointer is moved one element off its 16-byte boundary.  A test of its own,
test_overlap_contract, lays every output of every case over each activation input and each other output (abi_cases.check_overlap):
refused before anything is launched, or, for the pairs abi_cases.INPLACE declares, the bytes of the call on disjoint arrays.

Runners: a forward on a workspace that held garbage gives the logits of a forward on a clean one."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden, golden_scales

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import abi_cases as A  # noqa: E402
import ivit_amd as iv  # noqa: E402
from ivit_amd import _lib  # noqa: E402


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def twin():
    return A.load_twin()


cases_of = A.cases_of           # (label, args, setup, twinned) of every case of an entry in both tables, built once
NAMES = sorted(A.table_names()[0] | A.table_names()[1])


# (the completeness of the two tables and of abi_cases.ALIGN needs no device: tests/test_memory_contract_cpu.py)
@pytest.mark.parametrize("name", NAMES)
def test_memory_contract(H, twin, name):
    mem, host = A.TorchMem(), A.NumpyMem()
    fn = getattr(H.lib, "ivit_" + name)
    todo = cases_of(H, name)
    assert todo
    for label, args, setup, twinned in todo:
        what = f"ivit_{name} ({label})"
        refs, teardown = setup() if setup else (None, lambda: None)
        try:
            rows = A.TILE_ROWS_OF.get(name, A.TILE_ROWS)
            got = A.check_contract(fn, H.h, args, mem, refs, what, rows)             # checks 1 and 2
            want = A.plain_outputs(fn, H.h, args, mem, refs)                          # check 3
            for j, (g, w) in enumerate(zip(got, want)):
                assert np.array_equal(g, w), (what, "differs from the call on plain allocations", j, int((g != w).sum()))
            if twinned:
                href, keep = setup.host_refs(twin) if setup else (None, None)
                ref = A.plain_outputs(getattr(twin, "ivit_cpu_" + name), None, args, host, href)
                for j, (g, w) in enumerate(zip(got, ref)):
                    assert np.array_equal(g, w), (what, "differs from the CPU twin", j, int((g != w).sum()))
            for idx, outcome in A.ALIGN.get(name, {}).items():                        # check 4
                if args[idx] is not None:
                    A.check_alignment(fn, H, args, mem, refs, idx, outcome, got, what, rows)
        finally:
            teardown()


@pytest.mark.parametrize("name", NAMES)
def test_overlap_contract(H, name):
    """include/ivit.h, overlapping arguments: an array an entry writes laid over an activation input or over another array it writes
    is refused before anything is launched, unless abi_cases.INPLACE lists the pair (then the same pointer gives the bytes of the
    call on disjoint arrays, twice); arrays that merely touch are accepted.  Every case of both tables, every pair, every placement
    of abi_cases.overlap_placements, each inside one allocation of the test's own."""
    mem = A.TorchMem()
    fn = getattr(H.lib, "ivit_" + name)
    todo = cases_of(H, name)
    assert todo
    for label, args, setup, _ in todo:
        refs, teardown = setup() if setup else (None, lambda: None)
        try:
            A.check_overlap(fn, H, args, mem, refs, f"ivit_{name} ({label})", A.TILE_ROWS_OF.get(name, A.TILE_ROWS), name=name)
        finally:
            teardown()


# ---------------------------------------------------------------- the runners on a dirty workspace
def _vit(fname, scales=None):
    from ivit_amd.engine import ViTEngine
    g = load_golden(fname)
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    w = iv.make_vit_weights(cfg, int(g["seed"]))
    return g, cfg, w, ViTEngine.from_float(cfg, w, scales or golden_scales(g))


def _swin(fname):
    from ivit_amd.swin_engine import SwinEngine
    g = load_golden(fname)
    cfg = iv.SWIN_CONFIGS[str(g["cfg_name"])]
    return g, cfg, SwinEngine(cfg, iv.make_swin_weights(cfg, int(g["seed"])), golden_scales(g))


def _images(g, cfg, B):
    gb = int(g["batch"])
    imgs = np.concatenate([iv.make_images_int8(cfg, gb, int(g["images_seed"])), iv.make_images_int8(cfg, 4, seed=31)])[:B]
    return np.ascontiguousarray(imgs)


FILLS = ("0x00", "0xFF", "0x7F", "random")


def _dirty(ws, fill):
    if fill == "random":
        gen = torch.Generator(device="cuda").manual_seed(1234)
        ws.copy_(torch.randint(0, 256, (ws.numel(),), dtype=torch.uint8, device="cuda", generator=gen))
    else:
        ws.fill_(int(fill, 16))


def _dirty_workspace_forwards(eng, imgs, ns, want, golden_rows):
    """for each fill: the engine's own workspace of this (batch, slices) filled, initialised, two forwards back to back; all eight
    logits tensors equal `want` (when given) and each other, and the golden prefix equals the fixture"""
    B = imgs.shape[0]
    d = torch.from_numpy(imgs).cuda()
    ws, _ = eng._native_buffers(B, ns)
    got = {}
    for fill in FILLS:
        _dirty(ws, fill)
        eng._workspace_init(ws, B, ns)
        got[fill, 1] = eng.forward(d, nslices=ns).cpu().numpy()
        got[fill, 2] = eng.forward(d, nslices=ns).cpu().numpy()      # the v region now holds what the last layer stored there
    first = want if want is not None else got[FILLS[0], 1]
    for key, logits in got.items():
        assert np.array_equal(logits, first), (key, "rows that differ:", np.nonzero((logits != first).any(axis=1))[0].tolist())
    n = min(B, golden_rows.shape[0])
    assert np.array_equal(first[:n], golden_rows[:n])
    return d, ws, first


VIT_MODELS = ["micro_vit_b2.npz", "micro_vit2h_b3.npz", "deit_tiny_b1.npz"]
SWIN_MODELS = ["micro_swin_b2.npz", "micro_swin_w12_b2.npz"]


@pytest.mark.parametrize("B,ns", [(3, 2), (1, 1)])
@pytest.mark.parametrize("fname", VIT_MODELS + SWIN_MODELS)
def test_runner_on_dirty_workspace(fname, B, ns):
    """logits are a function of images and model only: B = 3 in two ragged slices (both on the larger slice's layout) and B = 1"""
    if fname in VIT_MODELS:
        g, cfg, _, eng = _vit(fname)
    else:
        g, cfg, eng = _swin(fname)
    _dirty_workspace_forwards(eng, _images(g, cfg, B), ns, None, g["logits_int"])


@pytest.mark.parametrize("fname", VIT_MODELS + SWIN_MODELS)
def test_graph_replay_on_dirty_workspace(fname):
    """the same through capture() and replay: the graph's workspace is dirtied and initialised between replays"""
    if fname in VIT_MODELS:
        g, cfg, _, eng = _vit(fname)
    else:
        g, cfg, eng = _swin(fname)
    B, ns = 3, 2
    d = torch.from_numpy(_images(g, cfg, B)).cuda()
    want = eng.forward(d, nslices=ns).cpu().numpy()
    n = min(B, int(g["batch"]))
    assert np.array_equal(want[:n], g["logits_int"][:n])
    replay = eng.capture(d, nstreams=ns)
    ws, _ = eng._native_buffers(B, ns)
    for fill in FILLS:
        torch.cuda.synchronize()
        _dirty(ws, fill)
        eng._workspace_init(ws, B, ns)
        torch.cuda.synchronize()
        for rep in (1, 2):
            got = replay().cpu().numpy()
            assert np.array_equal(got, want), (fill, rep, np.nonzero((got != want).any(axis=1))[0].tolist())


@pytest.mark.parametrize("B,ns", [(3, 2), (1, 1)])
def test_runner_on_dirty_workspace_mixed_shiftmax_forms(B, ns):
    """one ViT with blocks of both kinds: block 0 without a Shiftmax row table (v^T, whose pad columns the init zeroes), block 1 with
    one (v row-major into the same region).  micro_vit's scales with block 1's softmax scale replaced by a value of the scale sweep
    whose table lines fit 64 entries; the reference is the oracle."""
    from oracle import oracle as orc
    g = load_golden("micro_vit_b2.npz")
    scales = golden_scales(g)
    sweep = load_golden("scale_sweep.npz")["attn/scales"]
    has_rowtab = lambda s: iv.freeze.shiftmax_rowtable(iv.freeze.shiftmax_tables(np.float32(s))) is not None
    pick = [np.float32(s) for s in sweep if has_rowtab(s)]
    assert pick
    scales["blocks.1.attn.qact_attn1"] = pick[0]
    kinds = [has_rowtab(scales[f"blocks.{i}.attn.qact_attn1"]) for i in range(2)]
    assert kinds == [False, True], kinds
    g2, cfg, w, eng = _vit("micro_vit_b2.npz", scales)
    imgs = _images(g, cfg, B)
    want, _ = orc.OracleViT(cfg, w, scales).forward(imgs)
    _dirty_workspace_forwards(eng, imgs, ns, np.asarray(want), np.asarray(want))


@pytest.mark.parametrize("fname", ["micro_vit_b2.npz", "micro_swin_b2.npz"])
def test_runners_refuse_overlapping_arrays(fname):
    """the whole-model entries: images, workspace and logits of a forward, and idx / val of a predict against those three and each
    other, laid over one another are refused before anything is launched (status, message with both names, no byte of any buffer
    changed).  Every substituted pointer lies inside a buffer of the engine's own that holds the substituted extent, so a call that
    is wrongly not refused still addresses only memory the test owns; the unchanged call then gives the golden logits."""
    if fname in VIT_MODELS:
        g, cfg, _, eng = _vit(fname)
    else:
        g, cfg, eng = _swin(fname)
    B, ns, k = 2, 1, 3
    imgs = torch.from_numpy(_images(g, cfg, B)).cuda()
    eng._use_current_stream()
    args, _, (ws, logits, idx, val) = eng._args(imgs, ns, k)
    lib, P = eng.h.lib, (lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off))
    n_img, n_log, n_k = imgs.numel(), logits.numel() * 4, idx.numel() * 4
    assert ws.numel() >= 4096 + max(n_img, n_log) and n_log >= 16 + n_k and n_img >= n_k
    IMG, WS, LOG, IDX, VAL = 1, 4, 6, 9, 10                     # positions in the predict entries' argument list
    forward = [(IMG, P(ws), "images", "workspace"), (IMG, P(ws, 4096), "images", "workspace"), (LOG, P(ws, 4096), "workspace", "logits"),
               (LOG, P(imgs), "images", "logits")]
    predict = [(IDX, P(logits), "logits", "idx"), (VAL, P(logits, 16), "logits", "val"), (VAL, P(idx), "idx", "val"), (IDX, P(ws, 4096), "workspace", "idx"),
               (VAL, P(imgs), "images", "val")]
    bufs = (ws, logits, idx, val)
    for entry, n_args, table in (("_forward", 7, forward), ("_predict", 11, forward + predict)):
        fn = getattr(lib, eng.PREFIX + entry)
        for pos, ptr, name_a, name_b in table:
            for t, fill in zip(bufs, (0x5A, -7, -7, -7.0)):
                t.fill_(fill)
            torch.cuda.synchronize()
            call = list(args[:n_args])
            call[pos] = ptr
            st = fn(*call)
            msg = lib.ivit_last_error(eng.h.h).decode()
            torch.cuda.synchronize()
            assert st == _lib.IVIT_ERR_INVALID, (entry, pos, name_a, name_b, st)
            assert "overlap" in msg and name_a in msg and name_b in msg, msg
            for t, fill in zip(bufs, (0x5A, -7, -7, -7.0)):
                assert (t == fill).all(), (entry, pos, "a refused call wrote one of its arrays")
    eng._workspace_init(ws, B, ns)
    assert getattr(lib, eng.PREFIX + "_predict")(*args) == 0
    torch.cuda.synchronize()
    n = min(B, int(g["batch"]))
    assert np.array_equal(logits.cpu().numpy()[:n], g["logits_int"][:n])


def test_harness_sees_device_writes_and_reads_outside_the_arrays(H):
    """the device side of the harness on two planted calls, both inside the arenas' own allocations: ivit_widen_i8_i16 told one
    element more than the arrays hold stores one int16 behind its output (check 1), and with an output that has room for it the
    extra element is the byte behind its input (check 2)"""
    mem = A.TorchMem()
    fn = H.lib.ivit_widen_i8_i16
    x = np.arange(-100, 100, dtype=np.int8)
    n = x.size
    good = [("in", x), ("out", np.zeros(n, np.int16)), n]
    assert np.array_equal(A.check_contract(fn, H.h, good, mem)[0].view(np.int16), x.astype(np.int16))
    with pytest.raises(A.ContractError, match="2 bytes written BEHIND the output"):
        A.check_contract(fn, H.h, [("in", x), ("out", np.zeros(n, np.int16)), n + 1], mem)
    with pytest.raises(A.ContractError, match="2 bytes depend on what lies around the inputs"):
        A.check_contract(fn, H.h, [("in", x), ("out", np.zeros(n + 1, np.int16)), n + 1], mem)
