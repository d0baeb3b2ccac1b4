"""The runners' refusals, pinned: every eager runner entry of micro_vit_b2 and micro_swin_b2 at batch 2 — workspace_bytes, forward,
predict, score, features, hidden_states, ivit_vit_attention and ivit_swin_class_map in both of their modes — answers every call of
tests/runner_refusal_cases.py (each breaks exactly one rule) with the status and the full text of ivit_last_error recorded in
tests/golden/runner_refusals.json, launches nothing (no byte of any of the entry's arrays changes), and then runs the unmodified call
to the golden logits.  The record was made by tools/make_runner_refusals_fixture.py from the library of commit 5e8798f, the last
one in which every entry carried its own copy of these checks.

Two kinds of text in the record were then edited by hand: the index-list refusals of ivit_vit_attention, which that library worded
"blocks_host is null or nblocks outside 1 .. depth" and "blocks_host must be strictly ascending block indices in [0, depth)", read
"blocks_host must be 1 .. 2 strictly ascending indices in [0, 2)", the one text of the hidden_states entries' lists."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden_scales, load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import runner_refusal_cases as rc  # noqa: E402
from ivit_amd import _lib  # noqa: E402

with open(os.path.join(GOLDEN, "runner_refusals.json")) as _f:
    RECORD = json.load(_f)


@pytest.fixture(scope="module")
def models():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return {fname: rc.engine(fname, load_golden, golden_scales) for fname in rc.MODELS}


@pytest.mark.parametrize("fname,key", [(fname, key) for fname in rc.MODELS for key in sorted(RECORD[fname])])
def test_refusals_are_the_recorded_ones_and_launch_nothing(models, fname, key):
    g, cfg, eng, imgs = models[fname]
    specs = rc.entries(cfg, eng, imgs)
    assert sorted(specs) == sorted(RECORD[fname]), "the record and the entries differ: regenerate the fixture"
    symbol, params = specs[key]
    mem, _ = rc.arenas(params)
    before = {n: t.clone() for n, t in mem.items()}
    cases, want = rc.refusals(params, eng.MAX_SLICES), RECORD[fname][key]
    assert [name for name, _ in cases] == [row["case"] for row in want], "the record and the cases differ: regenerate the fixture"
    for (name, change), row in zip(cases, want):
        st, text = rc.run(eng, symbol, params, mem, change)
        assert st == row["status"], (key, name, st, text)
        assert row["error"] is None or text == row["error"], (key, name, text, row["error"])
    torch.cuda.synchronize()
    for n in mem:
        assert torch.equal(mem[n], before[n]), (key, f"a refused call wrote {n}")
    # the same arguments, nothing wrong with them
    if "workspace" in mem:
        eng._workspace_init(mem["workspace"], rc.B, 1)
    st, text = rc.run(eng, symbol, params, mem)
    torch.cuda.synchronize()
    assert st == _lib.IVIT_OK, (key, text)
    lg = rc.good_logits(params, mem, cfg.num_classes)
    assert lg is None or np.array_equal(lg, g["logits_int"]), key
