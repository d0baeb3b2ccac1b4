"""Linear probe without a GPU: include/ivit_probe.h declares one entry under version 1 beside eight unchanged headers, the binding
follows it and the build its mtime; the new kernels are in the gfx950 code object without scratch; `probe_stats_reference` on a
hand-written case; `fit` on synthetic int8 features (every held-out row classified by the QUANTISED head, the residual of the stated
system within the backward-error bound of a stable fp64 solve); `Head.from_float` is freeze's QuantLinear rule; two gloo ranks merge
their statistics into the one-process statistics."""
import ctypes
import os
import re
import shutil
import socket
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import ivit_amd as iv
from ivit_amd import _abi, _lib, freeze
from ivit_amd.predict import probe_fit_reference, probe_stats_reference, probe_system
from ivit_amd.probe import Head, ProbeStats, fit
from test_search_cpu import _prototypes_digest

ENTRIES = {"ivit_probe_accumulate": 10}


# ---------------------------------------------------------------- the ninth header and its binding
def test_probe_header_declares_entry_and_version():
    hdr = open(os.path.join(ROOT, "include", "ivit_probe.h")).read()
    assert re.search(r'#include "ivit\.h"', hdr)
    assert int(re.search(r"#define IVIT_PROBE_VERSION (\d+)", hdr).group(1)) == 1 == _lib.IVIT_PROBE_VERSION
    assert _abi.PROBE_ABI.constants == {"IVIT_PROBE_VERSION": 1}
    assert list(_abi.PROBE_ABI.functions) == list(ENTRIES)
    for name in ENTRIES:                                  # one "Alignment:" and one "Overlap:" line in front of every entry
        m = re.search(r"\bint %s\(" % name, hdr)
        front = hdr[hdr.rfind(";", 0, m.start()) + 1:m.start()]
        assert len(re.findall(r"\bAlignment:", front)) == 1 and len(re.findall(r"\bOverlap:", front)) == 1, name
    assert re.search(r"int\s+ivit_probe_accumulate\s*\(\s*ivit_handle\s+h\s*,\s*const\s+int8_t\s*\*\s*feat8\s*,\s*const\s+int64_t\s*\*\s*labels\s*,"
                     r"\s*int64_t\s+rows\s*,\s*int\s+dim\s*,\s*int\s+num_classes\s*,\s*int\s+splits\s*,\s*int64_t\s*\*\s*gram\s*,"
                     r"\s*int64_t\s*\*\s*class_sum\s*,\s*int64_t\s*\*\s*count\s*\)", hdr)


# the eight older headers: prototype count, version and sha256 of their prototypes (names, parameter types and names, in order).  The
# first seven digests are those test_modelfile_cpu.py pins; ivit_modelfile.h's was computed with the same function on the parent commit
OLDER_HEADERS = {"ivit.h": (99, 111, "6817c4e822691347e82f51942395393d315550b28b44df8fd32f8d739abd6b52"),
                 "ivit_eval.h": (5, 1, "b47eee22a4d967fa3efca30b6994987eecccbe61cf040a3608941660bf3bee07"),
                 "ivit_features.h": (5, 1, "cb523d76e256d935c2b277e969372ad9fbcde8cbdb97559fa7d84a6516f2159f"),
                 "ivit_attnmap.h": (4, 1, "2f429e1f49a79e9a910707d666d5d274831c1f49f0e8177fd51abf43952572f6"),
                 "ivit_classmap.h": (3, 1, "8da355354133cbf09e4e986c0bb6e4081b79ba6c60ac3fdb746cceec64bc3620"),
                 "ivit_hidden.h": (7, 1, "e32b2dd1cfd7fa95a32729c1e3b888b5f32d46680928bf55b727671ba8d2f93f"),
                 "ivit_search.h": (4, 1, "9eb19bc2c54d09c40ef4eee451c7ed84db075aa304ded29c967e5abbfc9c57cb"),
                 "ivit_modelfile.h": (9, 1, "cc004a1a3defcd124101e555c0ea3f5479b1b478141e709a622a4103294fac1c")}


def test_probe_entry_bound_and_exported_beside_unchanged_headers():
    iv.build()
    lib = _lib.load()
    P, I, L = _lib._P, _lib._I, ctypes.c_int64
    assert list(_lib.PROBE_SIGNATURES) == list(ENTRIES) == list(_lib.PROBE_RESTYPES)
    for name, nparams in ENTRIES.items():             # every bound name is exported, with the header's parameter count
        bound = getattr(lib, name)
        assert len(_lib.PROBE_SIGNATURES[name]) == nparams and bound.argtypes == _lib.PROBE_SIGNATURES[name] and bound.restype is I, name
    assert _lib.PROBE_SIGNATURES["ivit_probe_accumulate"] == [P, P, P, L, I, I, I, P, P, P]
    versions = (_lib.IVIT_VERSION, _lib.IVIT_EVAL_VERSION, _lib.IVIT_FEATURES_VERSION, _lib.IVIT_ATTNMAP_VERSION, _lib.IVIT_CLASSMAP_VERSION,
                _lib.IVIT_HIDDEN_VERSION, _lib.IVIT_SEARCH_VERSION, _lib.IVIT_MODELFILE_VERSION)
    abis = (_lib.ABI, _lib.EVAL_ABI, _lib.FEATURES_ABI, _lib.ATTNMAP_ABI, _lib.CLASSMAP_ABI, _lib.HIDDEN_ABI, _lib.SEARCH_ABI, _lib.MODELFILE_ABI)
    older = set()
    for (name, (count, version, digest)), abi, v in zip(OLDER_HEADERS.items(), abis, versions):
        assert len(abi.functions) == count and v == version and _prototypes_digest(abi) == digest, name
        text = open(os.path.join(ROOT, "include", name)).read()
        assert _prototypes_digest(_abi.parse(text) if name == "ivit.h" else _abi.parse(text, base=_lib.ABI)) == digest, name
        assert "ivit_probe" not in text, name
        older |= set(abi.functions)
    assert not set(ENTRIES) & older
    with pytest.raises(_abi.AbiError):                    # it names a handle of ivit.h: it parses only with ivit.h as its base
        _abi.parse(open(_abi.PROBE_HEADER).read())


def test_build_follows_the_probe_header():
    so = iv.build()
    assert os.path.getmtime(so) >= os.path.getmtime(_abi.PROBE_HEADER)
    assert "ivit_probe.h" in _lib.SOURCES and os.path.exists(os.path.join(ROOT, "i-vit_amd", "csrc", "ivit_probe.h"))
    src = open(os.path.join(ROOT, "i-vit_amd", "_lib.py")).read()
    assert re.search(r"newest = max\(.*_abi\.MODELFILE_HEADER, _abi\.PROBE_HEADER", src)


def test_probe_on_both_engines():
    import inspect
    from ivit_amd import dist, predict
    from ivit_amd.engine import ViTEngine
    from ivit_amd.native import NativeEngine
    from ivit_amd.swin_engine import SwinEngine
    for cls in (NativeEngine, ViTEngine, SwinEngine):
        assert list(inspect.signature(cls.probe_accumulate).parameters)[1:] == ["images", "labels", "stats", "nslices"], cls
        assert list(inspect.signature(cls.with_head).parameters)[1:] == ["head"], cls
    assert ViTEngine._with_head_engine is not NativeEngine._with_head_engine and SwinEngine._with_head_engine is not NativeEngine._with_head_engine
    assert list(inspect.signature(predict.probe_fit).parameters)[:5] == ["engine", "batches", "num_classes", "ridge", "transform"]
    assert inspect.signature(predict.probe_fit).parameters["ridge"].default == 1e-3 == inspect.signature(fit).parameters["ridge"].default
    assert callable(dist.probe_fit_sharded)


# ---------------------------------------------------------------- the kernels in the code object
def test_probe_kernels_in_code_object_without_scratch(tmp_path):
    from test_cabi_cpu import _device_code_object
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        readelf = shutil.which("llvm-readelf")
    assert readelf, "llvm-readelf not found"
    co = tmp_path / "dev.co"
    co.write_bytes(_device_code_object(iv.build()))
    notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True, check=True).stdout
    kernels = {}
    for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        scratch = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        spill = re.search(r"\.vgpr_spill_count:\s+(\d+)", blk)
        lds = re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk)
        if nm and scratch and spill and lds:
            kernels[nm.group(1)] = (int(scratch.group(1)), int(spill.group(1)), int(lds.group(1)))
    assert len(kernels) > 100, "code object metadata looks wrong"
    gram = [k for k in kernels if re.fullmatch(r"_Z\d+probe_gram_kernel\w+", k)]
    cls = sorted(k for k in kernels if re.fullmatch(r"_Z\d+probe_class_kernelILb[01]EE\w+", k))
    assert len(gram) == 1 and len(cls) == 2, (gram, cls)             # class sums: privatised in LDS / straight global adds
    # no scratch, no spills; the [column][row] image is static LDS: 256 columns of 80 bytes and 16 bytes per 16 columns
    assert kernels[gram[0]] == (0, 0, 256 * 80 + 16 * 16), kernels[gram[0]]
    for k in cls:                                                    # the privatised sums are dynamic LDS
        assert kernels[k] == (0, 0, 0), (k, kernels[k])


# ---------------------------------------------------------------- the numpy statements
def test_probe_stats_reference_hand_written_case():
    """3 rows x 64 features, one ignored label"""
    x = np.zeros((3, 64), np.int8)
    x[0, 0], x[0, 1], x[0, 63] = 2, -3, -128
    x[1, 0], x[1, 1] = 5, 7                              # ignored: label 2 of 2 classes
    x[2, 0], x[2, 63] = -1, 127
    gram, class_sum, count = probe_stats_reference(x, [1, 2, 1], 2)
    assert gram.dtype == class_sum.dtype == count.dtype == np.int64
    assert gram.shape == (64, 64) and class_sum.shape == (2, 64) and count.tolist() == [0, 2]
    want = np.zeros((64, 64), np.int64)
    want[0, 0], want[1, 1], want[63, 63] = 4 + 1, 9, 16384 + 16129
    want[0, 1] = want[1, 0] = -6
    want[0, 63] = want[63, 0] = -256 - 127
    want[1, 63] = want[63, 1] = 384
    assert np.array_equal(gram, want)
    cs = np.zeros((2, 64), np.int64)
    cs[1, 0], cs[1, 1], cs[1, 63] = 1, -3, -1
    assert np.array_equal(class_sum, cs)
    # the ignore labels: negative, num_classes, and values that alias a class in 32 bits
    g2, s2, c2 = probe_stats_reference(x, [-1, 2 ** 32 + 1, 2 ** 40], 2)
    assert not g2.any() and not s2.any() and not c2.any()
    g3, s3, c3 = probe_stats_reference(x, [0, 1, 1], 2)
    assert np.array_equal(g3, x.astype(np.int64).T @ x.astype(np.int64)) and c3.tolist() == [1, 2]
    assert np.array_equal(s3[1], x[1].astype(np.int64) + x[2]) and np.array_equal(s3[0], x[0].astype(np.int64))


def _synthetic(C, dim, amp, noise, rows, held=1000):
    """numpy default_rng(7): C prototypes uniform in +-amp; labels, then features = prototype + uniform noise in +-noise, clipped
    to int8; `held` held-out rows drawn the same way afterwards"""
    rng = np.random.default_rng(7)
    proto = rng.uniform(-amp, amp, size=(C, dim))

    def draw(n):
        lab = rng.integers(0, C, size=n)
        x = proto[lab] + rng.uniform(-noise, noise, size=(n, dim))
        return np.clip(np.rint(x), -128, 127).astype(np.int8), lab.astype(np.int64)
    return draw(rows), draw(held)


@pytest.mark.parametrize("C,dim,amp,noise,rows,ridge", [(5, 64, 40, 8, 600, 1e-3), (10, 192, 30, 20, 2000, 1e-3), (7, 64, 40, 8, 50, 1e-2)],
                         ids=["a", "b", "c_singular"])
def test_fit_on_synthetic_features(C, dim, amp, noise, rows, ridge):
    """Case c has fewer rows than features: the Gram matrix is singular and only the ridge makes the system solvable.
    1. the QUANTISED head (logits_reference times scale) classifies all 1000 held-out rows;
    2. the residual of the stated system: |A V^T - M^T|_F <= 64 dim 2^-52 |A|_F |V|_F, the backward-error form of a stable fp64
       solve with a margin of 64."""
    (x, lab), (hx, hlab) = _synthetic(C, dim, amp, noise, rows)
    stats = probe_stats_reference(x, lab, C)
    s_feat = np.float32(0.037)
    head = fit(stats, s_feat, ridge=ridge)
    assert head.w8.dtype == np.int8 and head.w8.shape == (C, dim) and head.b32.dtype == np.int32 and head.scale.dtype == np.float32
    logits = head.logits_reference(hx)
    assert logits.dtype == np.int32 and logits.shape == (1000, C)
    out = logits.astype(np.float64) * head.scale.astype(np.float64)[None, :]
    top2 = np.sort(out, axis=1)[:, -2:]
    print("held-out accuracy %.4f, smallest gap between best and second best %.3f" % (np.mean(out.argmax(1) == hlab), (top2[:, 1] - top2[:, 0]).min()))
    assert np.array_equal(out.argmax(1), hlab)
    A, M, mu, n = probe_system(*stats, ridge)
    V, b = probe_fit_reference(*stats, ridge)
    res = np.linalg.norm(A @ V.T - M.T)
    bound = 64 * dim * 2.0 ** -52 * np.linalg.norm(A) * np.linalg.norm(V)
    print("residual %.3e, bound %.3e, relative %.3e" % (res, bound, res / (np.linalg.norm(A) * np.linalg.norm(V))))
    assert res <= bound
    # fit is the reference's (V, b) through Head.from_float on the features' scale, and a ProbeStats gives what its triple gives
    want = Head.from_float((V / np.float64(s_feat)).astype(np.float32), b.astype(np.float32), s_feat)
    assert np.array_equal(head.w8, want.w8) and np.array_equal(head.b32, want.b32) and np.array_equal(head.scale.view(np.uint32), want.scale.view(np.uint32))
    same = fit(ProbeStats.from_numpy(*stats), s_feat, ridge=ridge)
    assert np.array_equal(same.w8, head.w8) and np.array_equal(same.b32, head.b32)
    assert np.allclose(b, np.bincount(lab, minlength=C) / n - V @ mu, rtol=0, atol=0)


def test_fit_gives_an_empty_class_zeros():
    (x, lab), _ = _synthetic(5, 64, 40, 8, 600)
    stats = probe_stats_reference(x, lab, 7)             # classes 5 and 6 have no row
    V, b = probe_fit_reference(*stats)
    assert not V[5:].any() and not b[5:].any() and V[:5].any()
    head = fit(stats, 0.05)
    assert not head.w8[5:].any() and not head.b32[5:].any()
    with pytest.raises(ValueError):
        probe_fit_reference(np.zeros((64, 64), np.int64), np.zeros((3, 64), np.int64), np.zeros(3, np.int64))


def test_head_from_float_is_the_quantlinear_rule():
    rng = np.random.default_rng(3)
    w = rng.standard_normal((6, 128)).astype(np.float32)
    w[2] = 0.0                                           # a zero weight row
    bias = rng.standard_normal(6).astype(np.float32)
    s_feat = np.float32(0.0421)
    head = Head.from_float(w, bias, s_feat)
    w8, s_w = freeze.quantize_weight(w)
    b32, s_b = freeze.quantize_bias(bias, s_w, s_feat)
    assert head.w8.dtype == np.int8 and np.array_equal(head.w8, w8) and not head.w8[2].any()
    assert np.array_equal(head.weight_scale.view(np.uint32), s_w.view(np.uint32))
    assert head.b32.dtype == np.int32 and np.array_equal(head.b32, b32)
    assert np.array_equal(head.scale.view(np.uint32), s_b.view(np.uint32)) and np.array_equal(s_b, (s_w * s_feat).astype(np.float32))
    assert head.num_classes == 6 and head.dim == 128 and head.feature_scale == float(s_feat)
    assert np.array_equal(head.weight, w) and np.array_equal(head.bias, bias)
    f = rng.integers(-128, 128, size=(9, 128)).astype(np.int8)
    want = f.astype(np.int64) @ w8.astype(np.int64).T + b32
    assert np.array_equal(head.logits_reference(f), want.astype(np.int32)) and np.array_equal(head.logits_reference(f)[:, 2], np.full(9, b32[2]))
    with pytest.raises(OverflowError):                   # |bias / (weight_scale * feature_scale)| >= 2^31
        Head.from_float(w, np.full(6, 1e9, np.float32), s_feat)
    with pytest.raises(ValueError):
        Head.from_float(w, bias[:5], s_feat)


def test_probe_stats_host_side():
    """construction, merge, numpy, zero_ work without a device; add does not"""
    rng = np.random.default_rng(1)
    x = rng.integers(-128, 128, size=(40, 64)).astype(np.int8)
    lab = rng.integers(-1, 4, size=40)
    a = ProbeStats.from_numpy(*probe_stats_reference(x[:25], lab[:25], 3))
    b = ProbeStats.from_numpy(*probe_stats_reference(x[25:], lab[25:], 3))
    a.merge(b).merge(probe_stats_reference(x[:0], lab[:0], 3))
    for got, want in zip(a.numpy(), probe_stats_reference(x, lab, 3)):
        assert got.dtype == np.int64 and np.array_equal(got, want)
    assert not any(t.any() for t in a.zero_().numpy())
    with pytest.raises(ValueError):
        ProbeStats(96, 3, "cpu")
    with pytest.raises(ValueError):
        ProbeStats(64, 0, "cpu")
    with pytest.raises(ValueError):
        a.merge(ProbeStats(128, 3, "cpu"))
    import torch
    with pytest.raises(iv.IvitError):
        ProbeStats(64, 3, "cpu").add(torch.from_numpy(x), torch.from_numpy(lab.astype(np.int64)))


# ---------------------------------------------------------------- two gloo ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _data():
    rng = np.random.default_rng(21)
    return rng.integers(-128, 128, size=(37, 64)).astype(np.int8), rng.integers(-1, 6, size=37).astype(np.int64)


def _worker(rank, world, port, q):
    import torch.distributed as dist
    from ivit_amd import dist as ivdist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    x, lab = _data()
    lo, hi = ivdist.shard_range(len(lab), rank, world)
    stats = ProbeStats.from_numpy(*probe_stats_reference(x[lo:hi], lab[lo:hi], 5)).all_reduce()
    q.put((rank,) + tuple(a.tobytes() for a in stats.numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_merge_into_the_one_process_statistics():
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = tuple(a.tobytes() for a in probe_stats_reference(*_data(), 5))
    assert res[0][1:] == want and res[1][1:] == want
