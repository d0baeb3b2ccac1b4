"""The stream and hipGraph contract of the C-ABI's operator entries (include/ivit.h, Conventions: "every call is asynchronous on the
handle's HIP stream, allocates nothing, synchronises nothing and is hipGraph-capturable"; the later headers inherit it).

Every case of both tables of tests/abi_cases.py, the two ragged front-end entries and the three entries of include/ivit_views.h go
through abi_cases.check_stream_contract: the handle is moved to a side stream and the call captured there; nothing may have run by the
time the device is synchronised (a launch that forgets the handle's stream has run by then: every other test keeps the handle on the
current stream and cannot tell); the graph must hold a node, replay to the bytes of the eager call, and replay on OTHER input contents
— the same case built from abi_cases.SECOND_SEED = 1234 — to the bytes of the eager call on those (a decision taken on the host from
device values would be baked into the graph).  With seed 1234 every case with an input array that differs between the seeds gives
outputs that differ too; none is exempted.

The harness is run on planted entries that break the contract, and a fresh process makes its first launches inside a capture."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import abi_cases as A  # noqa: E402
from ivit_amd import _lib  # noqa: E402
import pil_fixture  # noqa: E402
import pil_views_fixture  # noqa: E402


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib.Handle(0, torch.cuda.current_stream().cuda_stream)


NAMES = sorted(A.table_names()[0] | A.table_names()[1])


def _run_case(fn, H, args, args2, refs, what):
    """the harness on one case, and the non-vacuity of its step 5: where an input array differs, an output byte differs"""
    diffs, changed, _ = A.table_differences(args, args2)
    assert not diffs, (what, diffs)
    want1, want2 = A.check_stream_contract(fn, H, args, args2, A.TorchMem(), refs, what)
    if changed:
        assert any(not np.array_equal(a, b) for a, b in zip(want1, want2)), (what, "the second inputs give the first outputs: step 5 proves nothing")


@pytest.mark.parametrize("name", NAMES)
def test_stream_contract(H, name):
    fn = getattr(H.lib, "ivit_" + name)
    todo, other = A.cases_of(H, name), A.cases_of(H, name, second=True)
    assert todo and len(todo) == len(other)
    ran = 0
    for (label, args, setup, _), (label2, args2, _, _) in zip(todo, other):
        assert label == label2
        refs, teardown = setup() if setup else (None, lambda: None)       # plans and device constants stay those of the first table
        try:
            _run_case(fn, H, args, args2, refs, f"ivit_{name} ({label})")
            ran += 1
        finally:
            teardown()
    assert ran == len(A.cases_of(H, name))


# ---------------------------------------------------------------- the entries outside the tables
def _other_pixels(args, seed):
    """the same call on other pixel bytes: the descriptor tables (host and device) stay, by the entries' documented design the host
    table is read at call time"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return [("in", rng.integers(0, 256, args[0][1].shape, dtype=np.uint8))] + list(args[1:])


@pytest.mark.parametrize("nchw", [False, True], ids=["resize_center_crop_u8_pil", "eval_transform_u8"])
def test_stream_contract_of_the_ragged_front_end(H, nchw):
    _, images, cases = pil_fixture.fixture()
    size, crop, idx, _ = cases[0]
    name, args, keep = pil_fixture.entry_args([images[i] for i in idx], size, crop, nchw)
    _run_case(getattr(H.lib, name), H, args, _other_pixels(args, 7), None, name)


@pytest.mark.parametrize("nchw", [False, True], ids=["view_resize_u8_pil", "view_transform_u8"])
def test_stream_contract_of_the_view_entries(H, nchw):
    _, images, groups = pil_views_fixture.views_fixture()
    crop, views, _ = groups[0]
    name, args, keep = pil_views_fixture.entry_args(images, views, crop, nchw)
    _run_case(getattr(H.lib, name), H, args, _other_pixels(args, 8), None, name)


def test_stream_contract_of_logits_view_sum(H):
    """3 groups of 5 views of 10 classes; column 0 saturates at both ends in the first contents"""
    rngs = [np.random.default_rng(s) for s in (3, 4)]
    acc = [r.integers(-2**31, 2**31, size=(15, 10), dtype=np.int64).astype(np.int32) for r in rngs]
    acc[0][:5, 0], acc[0][5:10, 0] = np.iinfo(np.int32).max, np.iinfo(np.int32).min
    a1, a2 = ([("in", a), 3, 5, 10, ("out", np.zeros((3, 10), np.int32))] for a in acc)
    _run_case(H.lib.ivit_logits_view_sum, H, a1, a2, None, "ivit_logits_view_sum")


# ---------------------------------------------------------------- the harness on planted entries
def test_harness_catches_entries_that_break_the_stream_contract(H):
    """entries built from ivit_widen_i8_i16, no kernel of the test's own: the sound one passes; one launched through a second handle
    on a second stream runs at once; one that launches nothing; one that decides on the host, per call, which device buffer it
    reads.  Torch's pool streams are non-blocking and nothing here is launched on the default stream while a capture is open."""
    lib, mem = H.lib, A.TorchMem()
    n = 1000
    x1, x2 = np.arange(-500, 500).astype(np.int8), np.arange(500, -500, -1).astype(np.int8)
    args, args2 = ([("in", x), ("out", np.zeros(n, np.int16)), n] for x in (x1, x2))
    want1, want2 = A.check_stream_contract(lib.ivit_widen_i8_i16, H, args, args2, mem, None, "sound")
    assert np.array_equal(want1[0].view(np.int16), x1.astype(np.int16)) and np.array_equal(want2[0].view(np.int16), x2.astype(np.int16))

    elsewhere = torch.cuda.Stream()
    h2 = _lib.Handle(0, elsewhere.cuda_stream)

    def on_another_stream(h, x, out, n):
        return lib.ivit_widen_i8_i16(h2.h, x, out, n)
    # 2000 output bytes, of which the low bytes of 90, 346, -166 and -422 are the fill's 0x5A themselves
    with pytest.raises(A.ContractError, match="1996 bytes of output 0 written before the graph was launched"):
        A.check_stream_contract(on_another_stream, H, args, args2, mem, None, "another stream")
    torch.cuda.synchronize()
    h2.close()

    with pytest.raises(A.ContractError, match="launched nothing into the capture"):
        A.check_stream_contract(lambda h, x, out, n: 0, H, args, args2, mem, None, "no launch")

    const = [torch.from_numpy(x).cuda() for x in (x1, x2)]
    torch.cuda.synchronize()

    def host_decided(period):
        """reads const[(calls // period) % 2] whatever its input argument: the choice is made on the host at call time"""
        calls = [0]

        def entry(h, x, out, n):
            pick = const[(calls[0] // period) % 2]
            calls[0] += 1
            return lib.ivit_widen_i8_i16(h, ctypes.c_void_p(pick.data_ptr()), out, n)
        return entry
    # the harness calls an entry three times: eager, captured, eager on the second inputs.  A choice that changes with every call is
    # seen at the first replay; one that holds for the first two calls only once the graph is replayed on the second inputs
    with pytest.raises(A.ContractError, match="first replay differs from the eager call"):
        A.check_stream_contract(host_decided(1), H, args, args2, mem, None, "decided per call")
    with pytest.raises(A.ContractError, match="replay on new inputs gives the old outputs"):
        A.check_stream_contract(host_decided(2), H, args, args2, mem, None, "decided per two calls")
    # and the handle is back on the current stream after every failure: the sound entry still passes
    A.check_stream_contract(lib.ivit_widen_i8_i16, H, args, args2, mem, None, "sound, again")


# ---------------------------------------------------------------- a process whose first launches are captured
CHILD_TIMEOUT = 13          # seconds: five times one run of the child on an MI355X box, measured at 2.6 s (library load and torch's import)


def test_first_call_of_a_process_inside_a_capture():
    """tests/first_call_child.py as a fresh process, in this process's environment as it stands: the first launch the process makes
    of ivit_layernorm at 65 792 B of dynamic LDS, of ivit_attention_fused_rowlut and of ivit_layernorm_mlp_fused_planned is made
    inside a capture, on a handle that lives on a side stream; launch_dyn's hipFuncSetAttribute and the runtime's first-launch work
    both fall between begin and end.
    Observed on an MI355X (ROCm's HIP runtime, relaxed capture): the runtime ACCEPTS hipFuncSetAttribute under a capture; all three
    calls return IVIT_OK, nothing runs before the graph is launched, the replay equals the oracle (LayerNorm) or the later eager call,
    and the same graph follows new inputs.  So a kernel's first launch on a device may be a captured one, and this test pins it."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "first_call_child.py")], cwd=ROOT, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT)
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0, (r.returncode, lines, r.stderr[-2000:])
    assert [(ln["entry"], ln.get("ok")) for ln in lines] == [("layernorm", True), ("attention_fused_rowlut", True), ("layernorm_mlp_fused_planned", True)]
