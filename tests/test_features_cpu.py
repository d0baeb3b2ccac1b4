"""Features without a GPU: include/ivit_features.h declares the five entries and the three constants, they are bound under names of
their own and exported while ivit.h and ivit_eval.h and their bindings stay what they were, build() follows the new header, both
kernel forms are in the gfx950 code object, `features_reference` states the contract (the reference's fp32 tensor bit for bit; unit
rows from the exact sum of squares), and `embed` keeps the order of ragged batches on a stub engine."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
import ivit_amd as iv
from ivit_amd import _abi, _lib
from test_predict_cpu import _device_code_object

ENTRIES = {"ivit_features_f32": 7, "ivit_vit_features": 11, "ivit_swin_features": 11, "ivit_vit_features_graph_create": 12,
           "ivit_swin_features_graph_create": 12}


# ---------------------------------------------------------------- the third header and its binding
def test_features_header_declares_entries_and_constants():
    hdr = open(os.path.join(ROOT, "include", "ivit_features.h")).read()
    assert re.search(r'#include "ivit\.h"', hdr) and "vit_quant.py:271-273" in hdr and "swin_quant.py:553-555" in hdr
    assert "Alignment:" in hdr
    assert int(re.search(r"#define IVIT_FEATURES_VERSION (\d+)", hdr).group(1)) == 1 == _lib.IVIT_FEATURES_VERSION
    assert _abi.FEATURES_ABI.constants == {"IVIT_FEATURES_VERSION": 1, "IVIT_FEATURES_DEQUANT": 0, "IVIT_FEATURES_UNIT": 1}
    assert (_lib.IVIT_FEATURES_DEQUANT, _lib.IVIT_FEATURES_UNIT) == (0, 1)
    assert re.search(r"int\s+ivit_features_f32\s*\(\s*ivit_handle\s+h\s*,\s*const\s+int8_t\s*\*\s*feat8\s*,\s*int\s+batch\s*,\s*int\s+dim\s*,"
                     r"\s*float\s+scale\s*,\s*int\s+mode\s*,\s*float\s*\*\s*out\s*\)", hdr)
    tail = (r"const\s+int8_t\s*\*\s*images\s*,\s*int\s+batch\s*,\s*int\s+nslices\s*,\s*void\s*\*\s*workspace\s*,\s*size_t\s+bytes\s*,"
            r"\s*int32_t\s*\*\s*logits\s*,\s*int8_t\s*\*\s*feat8\s*,\s*float\s+scale\s*,\s*int\s+mode\s*,\s*float\s*\*\s*feat32")
    for kind in ("vit", "swin"):
        assert re.search(rf"int\s+ivit_{kind}_features\s*\(\s*ivit_{kind}\s+m\s*,\s*{tail}\s*\)", hdr), kind
        assert re.search(rf"int\s+ivit_{kind}_features_graph_create\s*\(\s*ivit_{kind}\s+m\s*,\s*{tail}\s*,\s*ivit_graph\s*\*\s*out\s*\)", hdr), kind


def test_features_entries_bound_and_exported_beside_unchanged_headers():
    import ctypes
    iv.build()
    lib = _lib.load()
    P, I, F = _lib._P, _lib._I, ctypes.c_float
    assert list(_abi.FEATURES_ABI.functions) == list(ENTRIES) == list(_lib.FEATURES_SIGNATURES) == list(_lib.FEATURES_RESTYPES)
    for name, nparams in ENTRIES.items():
        bound = getattr(lib, name)
        assert len(_lib.FEATURES_SIGNATURES[name]) == nparams and bound.argtypes == _lib.FEATURES_SIGNATURES[name] and bound.restype is I, name
    assert _lib.FEATURES_SIGNATURES["ivit_features_f32"] == [P, P, I, I, F, I, P]
    assert _lib.FEATURES_SIGNATURES["ivit_swin_features"] == [P, P, I, I, P, ctypes.c_size_t, P, P, F, I, P]
    assert _lib.FEATURES_SIGNATURES["ivit_vit_features_graph_create"] == _lib.FEATURES_SIGNATURES["ivit_vit_features"] + [P]
    # ivit.h: 99 prototypes at version 111; ivit_eval.h: its five at version 1; none of the new names in either
    hdr, ehdr = (open(os.path.join(ROOT, "include", n)).read() for n in ("ivit.h", "ivit_eval.h"))
    assert len(_lib.ABI.functions) == 99 and _lib.IVIT_VERSION == 111 and _abi.parse(hdr).functions.keys() == _lib.ABI.functions.keys()
    assert len(_lib.EVAL_ABI.functions) == 5 and _lib.IVIT_EVAL_VERSION == 1 and _lib.EVAL_ABI.constants == {"IVIT_EVAL_VERSION": 1}
    assert not set(ENTRIES) & (set(_lib.SIGNATURES) | set(_lib.EVAL_SIGNATURES))
    assert "_features" not in hdr and "_features" not in ehdr and "ivit_features.h" not in hdr + ehdr
    with pytest.raises(_abi.AbiError):                    # it names handles of ivit.h: it parses only with ivit.h as its base
        _abi.parse(open(_abi.FEATURES_HEADER).read())


def test_build_follows_the_features_header():
    so = iv.build()
    assert os.path.getmtime(so) >= os.path.getmtime(_abi.FEATURES_HEADER)
    assert "ivit_features.h" in _lib.SOURCES
    src = open(os.path.join(ROOT, "i-vit_amd", "_lib.py")).read()
    assert re.search(r"newest = max\(.*_abi\.EVAL_HEADER.*_abi\.FEATURES_HEADER", src)


def test_features_kernel_compiled_for_gfx950():
    co = _device_code_object(iv.build())
    # the dequantised form and the unit-length form
    assert re.search(rb"_Z\d+features_f32_kernelILb0EE", co) and re.search(rb"_Z\d+features_f32_kernelILb1EE", co)


# ---------------------------------------------------------------- features_reference: the contract in numpy
def test_features_reference_dequant_is_the_references_fp32_tensor():
    from ivit_amd.predict import features_reference
    g = load_golden("micro_vit_b2.npz")
    q, s = g["site/qact2"], g["scale/qact2"]
    assert q.dtype == np.int8 and q.shape == (2, 64)
    out = features_reference(q, s, 0)
    assert out.dtype == np.float32 and out.shape == q.shape
    want = (torch.from_numpy(q).to(torch.float32) * torch.tensor(float(s), dtype=torch.float32)).numpy()     # integer times scale, in fp32
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(out, features_reference(q, s))                                    # the default mode
    # one rounding, of the product: the float64 product rounded once gives the same bits
    assert np.array_equal(out, (q.astype(np.float64) * np.float64(s)).astype(np.float32))
    for bad in (0.0, -1.0, np.nan, np.inf):
        for mode in (0, 1):
            with pytest.raises(ValueError):
                features_reference(q, bad, mode)
    with pytest.raises(ValueError):
        features_reference(q, s, 2)


def test_features_reference_unit_rows():
    from ivit_amd.predict import features_reference
    rng = np.random.default_rng(11)
    q = rng.integers(-128, 128, size=(40, 192), dtype=np.int64).astype(np.int8)
    q[3] = 0                                                                               # a row of zeros
    q[4] = 0
    q[4, 17] = -128                                                                        # single non-zeros
    q[5] = 0
    q[5, 191] = 127
    u = features_reference(q, 0.05, 1)
    assert u.dtype == np.float32 and u.shape == q.shape
    norms = np.sqrt((u.astype(np.float64) ** 2).sum(axis=1))
    live = np.ones(40, bool)
    live[3] = False
    assert np.all(np.abs(norms[live] - 1.0) <= 2.0 ** -23), np.abs(norms[live] - 1.0).max()
    assert np.all(u[3] == 0) and not np.any(np.signbit(u[3])) and not np.isnan(u).any()
    assert u[4, 17] == -1.0 and np.count_nonzero(u[4]) == 1 and u[5, 191] == 1.0 and np.count_nonzero(u[5]) == 1
    # the scale cancels: any finite positive one gives the same bits
    for s in (1e-30, 0.02682777, 1.0, 3e30):
        assert np.array_equal(u.view(np.uint32), features_reference(q, s, 1).view(np.uint32))
    # the sign of every element is its integer's, the row's direction is the integers'
    assert np.array_equal(np.sign(u), np.sign(q.astype(np.float32)))


def test_features_reference_unit_at_perfect_squares_and_their_neighbours():
    """ss a perfect square gives exact quotients where q / sqrt(ss) is a binary fraction; ss one off a square must not be taken for
    it: the float64 root is exact or correctly rounded, never truncated to the integer root"""
    from ivit_amd.predict import features_reference
    dim = 64
    one = np.zeros((2, dim), np.int8)
    one[0, 5], one[1, 9] = 127, -127                                                       # ss = 127^2
    u = features_reference(one, 1.0, 1)
    assert u[0, 5] == 1.0 and u[1, 9] == -1.0
    ones = np.ones((1, dim), np.int8)                                                      # ss = dim = 8^2
    assert np.all(features_reference(ones, 1.0, 1) == np.float32(0.125))
    ones16 = np.ones((1, 16), np.int8)                                                     # ss = 16
    assert np.all(features_reference(ones16, 1.0, 1) == np.float32(0.25))
    for delta_col, ss in ((None, 64), (0, 63), (1, 67)):                                   # 64, 64 - 1, 64 + 3
        q = np.ones((1, dim), np.int8)
        if delta_col == 0:
            q[0, 0] = 0
        if delta_col == 1:
            q[0, 1] = 2
        assert int((q.astype(np.int64) ** 2).sum()) == ss
        u = features_reference(q, 1.0, 1)
        want = (q.astype(np.float64) / np.sqrt(np.float64(ss))).astype(np.float32)
        assert np.array_equal(u, want)
        assert (u[0, 5] == np.float32(0.125)) == (ss == 64)
    # the largest sum the entry admits: 65536 elements of -128, ss = 2^30 = (2^15)^2
    big = np.full((1, 65536), -128, np.int8)
    assert np.all(features_reference(big, 1.0, 1) == np.float32(-2.0 ** -8))


# ---------------------------------------------------------------- embed, with features = features_reference
class FeatureStub:
    """the pattern of test_predict_cpu.StubEngine: 'images' are the int8 feature rows themselves"""
    num_features = 32

    def __init__(self, scale=0.05):
        self.scale, self.calls = np.float32(scale), []

    def features(self, images, normalize=False):
        from ivit_amd.predict import features_reference
        q = np.asarray(images, dtype=np.int8)
        self.calls.append((len(q), bool(normalize)))
        return q, features_reference(q, self.scale, 1 if normalize else 0)


def test_embed_ragged_batches_in_order_and_empty():
    from ivit_amd.predict import embed, features_reference
    rng = np.random.default_rng(2)
    q = rng.integers(-128, 128, size=(9, 32), dtype=np.int64).astype(np.int8)
    eng = FeatureStub()
    out = embed(eng, [q[0:4], q[4:8], q[8:9]])                                             # ragged last batch
    assert isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.shape == (9, 32)
    assert eng.calls == [(4, True), (4, True), (1, True)]                                  # unit length is the default
    assert np.array_equal(out.numpy().view(np.uint32), features_reference(q, eng.scale, 1).view(np.uint32))      # order kept
    # (images, labels) pairs as evaluate takes them, a transform in front, the dequantised form
    eng = FeatureStub()
    out = embed(eng, [(q[a:a + 2] + 0, np.zeros(2)) for a in range(0, 8, 2)], transform=lambda x: x[::-1], normalize=False)
    want = np.concatenate([q[a:a + 2][::-1] for a in range(0, 8, 2)])
    assert eng.calls == [(2, False)] * 4
    assert np.array_equal(out.numpy().view(np.uint32), features_reference(want, eng.scale, 0).view(np.uint32))
    # no batches at all
    out = embed(FeatureStub(), iter(()))
    assert out.shape == (0, 32) and out.dtype == torch.float32


def test_engines_name_their_feature_scale_and_width():
    """what an engine is built from carries the scale of forward_features' output beside the frozen constants, which stay what they
    were: qact2 of a ViT in the fp32 scalars, qact3 of a Swin in the host part of the packed constants (so it rides a broadcast)"""
    from ivit_amd.engine import frozen_vit
    from ivit_amd.freeze import freeze_swin, freeze_vit
    from ivit_amd.swin_engine import pack_swin_constants, packed_swin
    from conftest import golden_scales
    g = load_golden("micro_vit_b2.npz")
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    w = iv.make_vit_weights(cfg, int(g["seed"]))
    consts, f32 = frozen_vit(cfg, w, golden_scales(g))
    plain_consts, plain = freeze_vit(cfg, w, golden_scales(g))
    assert np.float32(f32["feat.s"]) == g["scale/qact2"] and "feat.s" not in plain
    assert {k: v for k, v in f32.items() if k != "feat.s"} == plain and consts.keys() == plain_consts.keys()
    g = load_golden("micro_swin_b2.npz")
    cfg = iv.SWIN_CONFIGS[str(g["cfg_name"])]
    w = iv.make_swin_weights(cfg, int(g["seed"]))
    blob, table, host = packed_swin(cfg, w, golden_scales(g))
    blob0, table0, host0 = pack_swin_constants(freeze_swin(cfg, w, golden_scales(g)))
    assert host["feat.s"] == ("f", float(g["scale/qact3"])) and "feat.s" not in host0
    assert np.array_equal(blob, blob0) and table == table0 and {k: v for k, v in host.items() if k != "feat.s"} == host0
    assert cfg.num_features == cfg.embed_dim << (cfg.num_layers - 1)
