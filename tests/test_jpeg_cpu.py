"""JPEG input without a GPU: the numpy statement (ivit_amd/jpeg.py) against Pillow's bytes in tests/golden/jpeg.npz, every byte; the
refusals with their status and reason; include/ivit_jpeg.h beside twelve unchanged headers and its binding; and the host decoder
(csrc/ivit_jpeg_host.h) as a stand-alone program, plain against the numpy statement and under the address and undefined-behaviour
sanitizers over the fixtures, every prefix of the two smallest files and seeded single-byte corruptions."""
import ctypes
import functools
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
import ivit_amd as iv
from ivit_amd import _abi, _lib
from ivit_amd import jpeg as J
from test_range_cpu import OLDER_HEADERS as ELEVEN_OLDER
from test_search_cpu import _prototypes_digest

ENTRIES = {"ivit_jpeg_query_host": 7, "ivit_jpeg_entropy_decode_host": 6, "ivit_jpeg_workspace_bytes": 3, "ivit_jpeg_reconstruct_u8": 10}
# ivit_range.h's was computed with the same function on the parent commit
OLDER_HEADERS = dict(ELEVEN_OLDER, **{"ivit_range.h": (3, 1, "0d18dc6a4e8aae25ca7cc9d420708299335a5cd5cf99e5b43dc2179b524df671")})
SANITIZE = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@functools.lru_cache(None)
def golden():
    z = load_golden("jpeg.npz")
    return {k: z[k] for k in z.files}


@functools.lru_cache(None)
def decoded(name):
    return J.jpeg_coefficients_reference(golden()["jpg_" + name].tobytes())


def accepted():
    return [str(n) for n in golden()["accepted"]]


# ---------------------------------------------------------------- the numpy statement against Pillow
def test_fixture_covers_the_edges_and_is_small():
    g, names = golden(), accepted()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpeg.npz")) <= min(1 << 20, max(
        os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden")) if f != "jpeg.npz"))
    for w, h in ((1, 1), (7, 9), (8, 8), (9, 7), (16, 16), (17, 33), (53, 37), (64, 48)):
        for kind, q in (("noise", 30), ("noise", 85), ("noise", 100), ("grad", 30), ("grad", 85), ("grad", 100)):
            for s in ("s0", "s1", "s2", "grey"):
                assert "%dx%d_%s_q%d_%s" % (w, h, kind, q, s) in names
    for n in ("opt_s0", "opt_s2", "rst1_s0", "rst2_s2", "rst1_grey", "long_app_trailing", "no_jfif", "adobe_ycc", "sof1", "q100_noise_big"):
        assert n in names
    samplings = {(decoded(n)[0].ncomp, decoded(n)[0].hs, decoded(n)[0].vs) for n in names}
    assert samplings == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    assert len(g["jpg_long_app_trailing"]) > 65535 and bytes(g["jpg_long_app_trailing"][-3:]) == b"\xff\xd8\xff"
    for n in ("progressive", "cmyk", "dqt255", "trunc_0"):
        assert n in g["refused"]


def test_jpeg_reference_is_pillow_on_every_accepted_fixture():
    g = golden()
    for n in accepted():
        info, coefs = decoded(n)
        out = J.reconstruct_reference(info, coefs)
        want = g["rgb_" + n]
        assert out.dtype == np.uint8 and out.shape == want.shape == (info.h, info.w, 3), n
        assert np.array_equal(out, want), (n, int((out != want).sum()))


def test_refusals_give_the_documented_status_and_reason():
    g = golden()
    seen = set()
    for n, st, why in zip(g["refused"], g["refused_status"], g["refused_reason"]):
        with pytest.raises(J.JpegRefused) as e:
            J.jpeg_reference(g["jpg_" + n].tobytes())
        assert e.value.status == int(st) and str(why) in str(e.value) and str(e.value), (n, str(e.value))
        seen.add(int(st))
    assert seen == {J.IVIT_ERR_INVALID, J.IVIT_ERR_UNSUPPORTED} == {_lib.IVIT_ERR_INVALID, _lib.IVIT_ERR_UNSUPPORTED}


def test_the_bound_refuses_the_patched_tables_and_no_quality_100_file():
    """the host's bound (csrc/ivit_jpeg_host.h): the file whose DQT bytes were set to 255 overshoots it — Pillow's own bytes for it
    are not the C arithmetic's, which is why it is refused — and nothing Pillow writes at quality 100 comes near it"""
    g = golden()
    with pytest.raises(J.JpegRefused) as e:
        J.jpeg_coefficients_reference(g["jpg_dqt255"].tobytes())
    assert e.value.status == J.IVIT_ERR_UNSUPPORTED and "bound" in str(e.value)
    q100 = [n for n in accepted() if "q100" in n]
    assert len(q100) >= 60 and "q100_noise_big" in q100 and "extremes_q100" in q100
    worst = 0
    for n in q100:
        info, coefs = decoded(n)
        for c in range(info.ncomp):
            assert (info.qt[c] == 1).all()                 # quality 100: the coefficients are the dequantised ones
            deq = coefs[c].astype(np.int64) * info.qt[c].astype(np.int64)
            worst = max(worst, int(np.abs(deq).reshape(-1, 8, 8).sum(1).max()))
            s = J._idct_samples(deq)
            assert -512 <= s.min() and s.max() <= 511
    assert 1000 < worst <= J.COLUMN_BOUND          # the fixture comes within a factor of three of the bound and stays inside


def test_range_limit_closed_form_is_the_masked_table():
    """libjpeg's table behind the IDCT (prepare_range_limit_table), indexed by the 10-bit masked sample: 128 .. 255, then 255, then 0,
    then 0 .. 127 — wrap-around included"""
    table = np.concatenate([np.arange(128, 256), np.full(384, 255), np.zeros(384, np.int64), np.arange(0, 128)])
    x = np.arange(-4096, 4096)
    v = x & 1023
    closed = np.clip(np.where(v >= 512, v - 1024, v) + 128, 0, 255)
    assert np.array_equal(closed, table[v])
    one = np.zeros((1, 64), np.int16)
    one[0, 0] = 8 * 700                                    # a flat block 700 above the centre wraps to 0
    assert (J.idct_reference(one, np.ones(64, np.uint8)) == 0).all()


# ---------------------------------------------------------------- the thirteenth header and its binding
def test_jpeg_header_declares_entries_and_version():
    hdr = open(os.path.join(ROOT, "include", "ivit_jpeg.h")).read()
    assert re.search(r'#include "ivit\.h"', hdr)
    assert int(re.search(r"#define IVIT_JPEG_VERSION (\d+)", hdr).group(1)) == 1 == _lib.IVIT_JPEG_VERSION
    assert _abi.JPEG_ABI.constants == {"IVIT_JPEG_VERSION": 1}
    assert list(_abi.JPEG_ABI.functions) == list(ENTRIES)
    for name in ENTRIES:                                  # one "Alignment:" and one "Overlap:" line in front of every entry
        m = re.search(r"\bint %s\(" % name, hdr)
        front = hdr[hdr.rfind(";", 0, m.start()) + 1:m.start()]
        assert len(re.findall(r"\bAlignment:", front)) == 1 and len(re.findall(r"\bOverlap:", front)) == 1, name
    fields = _abi.JPEG_ABI.structs["ivit_jpeg_desc"]
    assert tuple(d.name for d in fields) == J.JPEG_DESC_FIELDS
    assert [(d.base, d.array) for d in fields] == [("int64_t", None)] * 3 + [("int32_t", None)] * 5 + [("int32_t", 3)] * 2 + [
        ("int32_t", None), ("uint8_t", 192)]
    assert ctypes.sizeof(_lib.JpegDesc) == 264 and _lib.JpegDesc.qt.offset == 72 and _lib.JpegDesc.bw.offset == 44
    fns = _abi.JPEG_ABI.functions
    assert [p.name for p in fns["ivit_jpeg_query_host"].params] == ["data_host", "bytes", "desc_host", "coef_count", "workspace_bytes", "err_host",
                                                                    "err_bytes"]
    assert [p.name for p in fns["ivit_jpeg_entropy_decode_host"].params] == ["data_host", "bytes", "coefs_host", "coef_capacity", "err_host",
                                                                             "err_bytes"]
    assert [p.name for p in fns["ivit_jpeg_workspace_bytes"].params] == ["desc_host", "B", "bytes"]
    assert [p.name for p in fns["ivit_jpeg_reconstruct_u8"].params] == ["h", "coefs", "coef_count", "desc_host", "desc_dev", "B", "workspace",
                                                                        "workspace_bytes", "pixels", "pixels_bytes"]


def test_jpeg_entries_bound_and_exported_beside_unchanged_headers():
    iv.build()
    lib = _lib.load()
    P, I, L, Z = _lib._P, _lib._I, ctypes.c_int64, ctypes.c_size_t
    assert list(_lib.JPEG_SIGNATURES) == list(ENTRIES) == list(_lib.JPEG_RESTYPES)
    for name, nparams in ENTRIES.items():
        bound = getattr(lib, name)
        assert len(_lib.JPEG_SIGNATURES[name]) == nparams and bound.argtypes == _lib.JPEG_SIGNATURES[name] and bound.restype is I, name
    assert _lib.JPEG_SIGNATURES["ivit_jpeg_query_host"] == [P, Z, P, P, P, P, Z]
    assert _lib.JPEG_SIGNATURES["ivit_jpeg_entropy_decode_host"] == [P, Z, P, L, P, Z]
    assert _lib.JPEG_SIGNATURES["ivit_jpeg_workspace_bytes"] == [P, I, P]
    assert _lib.JPEG_SIGNATURES["ivit_jpeg_reconstruct_u8"] == [P, P, L, P, P, I, P, Z, P, Z]
    versions = (_lib.IVIT_VERSION, _lib.IVIT_EVAL_VERSION, _lib.IVIT_FEATURES_VERSION, _lib.IVIT_ATTNMAP_VERSION, _lib.IVIT_CLASSMAP_VERSION,
                _lib.IVIT_HIDDEN_VERSION, _lib.IVIT_SEARCH_VERSION, _lib.IVIT_MODELFILE_VERSION, _lib.IVIT_PROBE_VERSION, _lib.IVIT_VIEWS_VERSION,
                _lib.IVIT_CLUSTER_VERSION, _lib.IVIT_RANGE_VERSION)
    abis = (_lib.ABI, _lib.EVAL_ABI, _lib.FEATURES_ABI, _lib.ATTNMAP_ABI, _lib.CLASSMAP_ABI, _lib.HIDDEN_ABI, _lib.SEARCH_ABI, _lib.MODELFILE_ABI,
            _lib.PROBE_ABI, _lib.VIEWS_ABI, _lib.CLUSTER_ABI, _lib.RANGE_ABI)
    assert len(OLDER_HEADERS) == 12 == len(abis)
    older = set()
    for (name, (count, version, digest)), abi, v in zip(OLDER_HEADERS.items(), abis, versions):
        assert len(abi.functions) == count and v == version and _prototypes_digest(abi) == digest, name
        text = open(os.path.join(ROOT, "include", name)).read()
        assert _prototypes_digest(_abi.parse(text) if name == "ivit.h" else _abi.parse(text, base=_lib.ABI)) == digest, name
        assert "ivit_jpeg" not in text, name
        older |= set(abi.functions)
    assert not set(ENTRIES) & older
    with pytest.raises(_abi.AbiError):                    # it names a handle of ivit.h: it parses only with ivit.h as its base
        _abi.parse(open(_abi.JPEG_HEADER).read())


def test_build_follows_the_jpeg_header():
    so = iv.build()
    assert os.path.getmtime(so) >= os.path.getmtime(_abi.JPEG_HEADER)
    for f in ("ivit_jpeg.h", "ivit_jpeg_host.h"):
        assert f in _lib.SOURCES and os.path.exists(os.path.join(ROOT, "i-vit_amd", "csrc", f))
    src = open(os.path.join(ROOT, "i-vit_amd", "_lib.py")).read()
    assert re.search(r"newest = max\(.*_abi\.RANGE_HEADER, _abi\.JPEG_HEADER", src)
    hip = open(os.path.join(ROOT, "i-vit_amd", "csrc", "ivit_hip.hip")).read()
    assert '#include "ivit_jpeg.h"' in hip and '#include "ivit_jpeg_host.h"' in hip
    host = open(os.path.join(ROOT, "i-vit_amd", "csrc", "ivit_jpeg_host.h")).read()
    assert "hip" not in re.sub(r"//.*", "", host).lower() and "malloc" not in host and "new " not in re.sub(r"//.*", "", host)


def test_library_host_entries_are_the_numpy_statement():
    """the two host entries of the built library (no GPU call in either): descriptor, counts and every coefficient"""
    iv.build()
    g = golden()
    for n in accepted()[::7] + ["long_app_trailing", "rst2_s2", "opt_grey"]:
        data = g["jpg_" + n].tobytes()
        info, coefs = decoded(n)
        desc, ncoef, nws = J.query(data)
        assert (desc.w, desc.h, desc.ncomp, desc.hs, desc.vs) == (info.w, info.h, info.ncomp, info.hs, info.vs), n
        assert list(desc.bw)[:info.ncomp] == info.bw and list(desc.bh)[:info.ncomp] == info.bh and ncoef == nws == 64 * sum(info.blocks)
        assert (desc.coef_offset, desc.pixel_offset, desc.plane_offset, desc.reserved) == (0, 0, 0, 0)
        assert np.array_equal(np.frombuffer(bytes(desc.qt), np.uint8)[:64 * info.ncomp].reshape(-1, 64), info.qt)
        guard = np.full(ncoef + 16, 0x5A5A, np.int16)
        _, got = J.entropy_decode(data, guard[8:8 + ncoef])
        assert np.array_equal(got, np.concatenate([c.reshape(-1) for c in coefs])), n
        assert (guard[:8] == 0x5A5A).all() and (guard[8 + ncoef:] == 0x5A5A).all()
    with pytest.raises(J.JpegRefused) as e:
        J.query(g["jpg_progressive"].tobytes())
    assert e.value.status == J.IVIT_ERR_UNSUPPORTED and "progressive" in str(e.value)
    lib = _lib.load()
    data = g["jpg_8x8_noise_q85_s0"].tobytes()
    err = ctypes.create_string_buffer(64)
    small = np.zeros(8, np.int16)
    assert lib.ivit_jpeg_entropy_decode_host(data, len(data), ctypes.c_void_p(small.ctypes.data), 8, err, 64) == _lib.IVIT_ERR_INVALID
    assert b"room for 8" in err.value and not small.any()


# ---------------------------------------------------------------- the host decoder as a stand-alone program
def _cxx():
    return os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def _run_host(exe, streams, tmp_path, tag):
    src, dst = tmp_path / (tag + ".in"), tmp_path / (tag + ".out")
    with open(src, "wb") as f:
        for s in streams:
            f.write(struct.pack("<I", len(s)) + s)
    run = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-2000:])
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr and run.stderr.strip() == "", run.stderr[-2000:]
    out, pos, res = dst.read_bytes(), 0, []
    for _ in streams:
        st = struct.unpack_from("<i", out, pos)[0]
        pos += 4
        if st == 0:
            head = struct.unpack_from("<11i", out, pos)
            qt = np.frombuffer(out, np.uint8, 192, pos + 44)
            n = struct.unpack_from("<q", out, pos + 236)[0]
            res.append((st, head, qt, np.frombuffer(out, np.int16, n, pos + 244)))
            pos += 244 + 2 * n
        else:
            res.append((st, None, None, None))
    assert pos == len(out)
    return res


def test_host_program_plain_build_is_the_numpy_statement(tmp_path):
    cxx = _cxx()
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "jpeg_host_main")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "jpeg_host_main.cc"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    g = golden()
    names = accepted() + [str(n) for n in g["refused"]]
    res = _run_host(exe, [g["jpg_" + n].tobytes() for n in names], tmp_path, "fixtures")
    status = dict(zip((str(n) for n in g["refused"]), (int(s) for s in g["refused_status"])))
    for n, (st, head, qt, coefs) in zip(names, res):
        assert st == status.get(n, 0), n
        if st == 0:
            info, want = decoded(n)
            pad = [0] * (3 - info.ncomp)
            assert head == (info.w, info.h, info.ncomp, info.hs, info.vs, *info.bw, *pad, *info.bh, *pad), n
            assert np.array_equal(qt[:64 * info.ncomp].reshape(-1, 64), info.qt) and not qt[64 * info.ncomp:].any(), n
            assert np.array_equal(coefs, np.concatenate([c.reshape(-1) for c in want])), n


def test_host_program_sanitised_over_fixtures_prefixes_and_corruptions(tmp_path):
    """address + undefined-behaviour sanitizers on the stand-alone program (nothing is loaded into Python): every fixture, every
    prefix of the two smallest files, 300 seeded single-byte corruptions of one file.  Every stream is decoded or refused with a
    status and a reason, the program exits 0 and the sanitizers report nothing; a decoded stream equals the numpy statement's
    verdict.  Skips only where a one-line sanitised program does not build."""
    cxx = _cxx()
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if not cxx or subprocess.run([cxx] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no host compiler builds a sanitised program here")
    exe = str(tmp_path / "jpeg_host_main_san")
    subprocess.run([cxx] + SANITIZE + [os.path.join(ROOT, "tests", "jpeg_host_main.cc"), "-o", exe], check=True, capture_output=True, timeout=300)
    g = golden()
    names = accepted() + [str(n) for n in g["refused"]]
    fixtures = [g["jpg_" + n].tobytes() for n in names]
    smallest = sorted((g["jpg_" + n].tobytes() for n in accepted()), key=len)[:2]
    prefixes = [s[:k] for s in smallest for k in range(len(s))]
    rng = np.random.default_rng(2024)
    victim = bytearray(g["jpg_rst2_s2"].tobytes())
    corrupt = []
    for _ in range(300):
        b = bytearray(victim)
        b[int(rng.integers(2, len(b)))] = int(rng.integers(0, 256))
        corrupt.append(bytes(b))
    res = _run_host(exe, fixtures + prefixes + corrupt, tmp_path, "all")
    status = dict(zip((str(n) for n in g["refused"]), (int(s) for s in g["refused_status"])))
    assert [r[0] for r in res[:len(names)]] == [status.get(n, 0) for n in names]
    assert all(r[0] == J.IVIT_ERR_INVALID for r in res[len(names):len(names) + len(prefixes)])       # no proper prefix is a file
    for s, r in list(zip(corrupt, res[len(names) + len(prefixes):]))[::10]:                          # the numpy statement agrees
        try:
            _, want = J.jpeg_coefficients_reference(s)
            assert r[0] == 0 and np.array_equal(r[3], np.concatenate([c.reshape(-1) for c in want]))
        except J.JpegRefused as e:
            assert r[0] == e.status
    assert {r[0] for r in res[len(names) + len(prefixes):]} >= {0, J.IVIT_ERR_INVALID}


def test_classify_jpeg_example_compiles_against_the_headers(tmp_path):
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc")
    assert cc, "no host C compiler"
    src = os.path.join(ROOT, "examples", "classify_jpeg.c")
    subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                    "-D__HIP_PLATFORM_AMD__", "-c", src, "-o", str(tmp_path / "classify_jpeg.o")], check=True, capture_output=True, timeout=120)
    text = open(src).read()
    for fn in ("ivit_jpeg_query_host", "ivit_jpeg_entropy_decode_host", "ivit_jpeg_reconstruct_u8", "ivit_eval_transform_u8", "_predict"):
        assert fn in text
