"""The device entropy decode without a GPU: include/ivit_jpeg_entropy.h beside thirteen unchanged headers and its binding; the host
pre-pass (csrc/ivit_jpeg_scan_host.h) against the numpy statement (ivit_amd/jpeg.py, jpeg_scan_reference) on every golden file, with
the refusals' statuses and reasons; and the pre-pass as a stand-alone program, plain and under the address and undefined-behaviour
sanitizers, over the golden files and every one-byte truncation of three of them."""
import ctypes
import functools
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT, load_golden
import ivit_amd as iv
from ivit_amd import _abi, _lib
from ivit_amd import jpeg as J
from test_jpeg_cpu import OLDER_HEADERS as TWELVE_OLDER, SANITIZE, _cxx
from test_search_cpu import _prototypes_digest

ENTRIES = {"ivit_jpeg_scan_host": 12, "ivit_jpeg_entropy_workspace_bytes": 3, "ivit_jpeg_entropy_decode": 17}
# ivit_jpeg.h's was computed with the same function on the parent commit
OLDER_HEADERS = dict(TWELVE_OLDER, **{"ivit_jpeg.h": (4, 1, "72d8bd5749609cbee110ee1d9e5cb6f40c2c255380e1a5fafde8dba1342089da")})


@functools.lru_cache(None)
def files():
    """name -> bytes of every golden file, accepted and refused, of both fixtures"""
    g, e = load_golden("jpeg.npz"), load_golden("jpeg_entropy.npz")
    out = {str(n): g["jpg_" + str(n)].tobytes() for n in list(g["accepted"]) + list(g["refused"])}
    out.update((str(n), e["jpg_" + str(n)].tobytes()) for n in e["names"])
    return out


def test_entropy_header_version_binding_and_older_digests():
    hdr = open(_abi.JPEG_ENTROPY_HEADER).read()
    assert re.search(r'#include "ivit_jpeg\.h"', hdr) and "several workgroups per file" in hdr and "unstuffing on" in hdr
    assert int(re.search(r"#define IVIT_JPEG_ENTROPY_VERSION (\d+)", hdr).group(1)) == 1 == _lib.IVIT_JPEG_ENTROPY_VERSION
    assert list(_abi.JPEG_ENTROPY_ABI.functions) == list(ENTRIES) == list(_lib.JPEG_ENTROPY_SIGNATURES) == list(_lib.JPEG_ENTROPY_RESTYPES)
    for name in ENTRIES:                                  # one "Alignment:" and one "Overlap:" line in front of every entry
        m = re.search(r"\bint %s\(" % name, hdr)
        front = hdr[hdr.rfind(";", 0, m.start()) + 1:m.start()]
        assert len(re.findall(r"\bAlignment:", front)) == 1 and len(re.findall(r"\bOverlap:", front)) == 1, name
    assert (ctypes.sizeof(_lib.JpegSegment), ctypes.sizeof(_lib.JpegHuff), ctypes.sizeof(_lib.JpegScan)) == (24, 1484, 6008)
    assert _lib.JpegScan.dc.offset == 72 and J.SEGMENT_DTYPE.itemsize == 24
    iv.build()
    lib = _lib.load()
    for name, nparams in ENTRIES.items():
        bound = getattr(lib, name)
        assert len(_lib.JPEG_ENTROPY_SIGNATURES[name]) == nparams and bound.argtypes == _lib.JPEG_ENTROPY_SIGNATURES[name], name
    assert os.path.getmtime(_lib.SO_PATH) >= os.path.getmtime(_abi.JPEG_ENTROPY_HEADER)
    assert re.search(r"newest = max\(.*_abi\.JPEG_HEADER, _abi\.JPEG_ENTROPY_HEADER", open(os.path.join(ROOT, "i-vit_amd", "_lib.py")).read())
    abis = (_lib.ABI, _lib.EVAL_ABI, _lib.FEATURES_ABI, _lib.ATTNMAP_ABI, _lib.CLASSMAP_ABI, _lib.HIDDEN_ABI, _lib.SEARCH_ABI, _lib.MODELFILE_ABI,
            _lib.PROBE_ABI, _lib.VIEWS_ABI, _lib.CLUSTER_ABI, _lib.RANGE_ABI, _lib.JPEG_ABI)
    assert len(OLDER_HEADERS) == 13 == len(abis)
    for (name, (count, version, digest)), abi in zip(OLDER_HEADERS.items(), abis):
        assert len(abi.functions) == count and _prototypes_digest(abi) == digest, name
        assert [v for k, v in abi.constants.items() if k.endswith("_VERSION")][0] == version, name
        text = open(os.path.join(ROOT, "include", name)).read()
        assert "ivit_jpeg_entropy.h" not in text and not any(re.search(r"\b%s\b" % e, text) for e in ENTRIES), name
        assert not set(ENTRIES) & set(abi.functions)


def test_scan_host_is_the_numpy_statement_on_every_golden_file():
    iv.build()
    scanned = 0
    for name, data in files().items():
        try:
            want_stream, want_segs = J.jpeg_scan_reference(data)
        except J.JpegRefused as want:
            with pytest.raises(J.JpegRefused) as e:
                J.scan(data)
            assert e.value.status == want.status and e.value.reason == want.reason, name
            continue
        guard = np.full(len(data) + 64, 0x5A, np.uint8)
        desc, rec, stream, segs, ncoef, nws = J.scan(data, guard[32:32 + len(data)])
        pad = -len(stream) % 8
        assert np.array_equal(stream, want_stream) and np.array_equal(segs, want_segs), name
        assert (guard[:32] == 0x5A).all() and not guard[32 + len(stream):32 + len(stream) + pad].any() and (guard[32 + len(stream) + pad:] == 0x5A).all()
        q = J.query(data)
        assert bytes(desc) == bytes(q[0]) and (ncoef, nws) == q[1:] and rec.stream_bytes == len(stream) and rec.segment_count == len(segs), name
        assert (rec.stream_offset, rec.work_offset, rec.segment_offset, *rec.reserved) == (0, 0, 0, 0, 0) and max(*rec.td, *rec.ta) <= 1
        for t in (rec.dc[0], rec.ac[0]):                       # the look-ahead table restates the codes of up to 9 bits
            lut, n = np.array(t.lut), 0
            for length in range(1, 10):
                for code in range(t.mincode[length], t.maxcode[length] + 1):
                    entries = lut[code << (9 - length):(code + 1) << (9 - length)]
                    assert (entries == (length << 8 | t.vals[t.valptr[length] + code - t.mincode[length]])).all()
                    n += len(entries)
            assert n == np.count_nonzero(lut)
        scanned += 1
    g = load_golden("jpeg.npz")
    assert scanned == len(g["accepted"]) + len(load_golden("jpeg_entropy.npz")["names"]) + 1          # and dqt255: its refusal is the device's
    with pytest.raises(J.JpegRefused) as e:                    # every capacity is checked
        J.scan(files()["rst1_s0"], np.zeros(64, np.uint8))
    assert e.value.status == J.IVIT_ERR_INVALID and "room for" in e.value.reason


@pytest.mark.parametrize("flags", [["-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror"], SANITIZE], ids=["plain", "sanitised"])
def test_scan_program_over_golden_files_and_truncations(tmp_path, flags):
    """tests/jpeg_scan_main.cc as a child process (nothing is loaded into Python): every golden file, and every proper prefix of three
    of them; statuses, sizes and checksums are the numpy statement's, every prefix is refused, the sanitizers report nothing"""
    cxx = _cxx()
    assert cxx, "no host C++ compiler"
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if flags is SANITIZE and subprocess.run([cxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no host compiler builds a sanitised program here")
    exe = str(tmp_path / "jpeg_scan_main")
    subprocess.run([cxx] + flags + [os.path.join(ROOT, "tests", "jpeg_scan_main.cc"), "-o", exe], check=True, capture_output=True, timeout=300)
    paths = []
    for name, data in files().items():
        paths.append(str(tmp_path / (name + ".jpg")))
        with open(paths[-1], "wb") as f:
            f.write(data)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and run.stderr.strip() == "", run.stderr[-2000:]
    lines = run.stdout.split("\n")
    for (name, data), line in zip(files().items(), lines):
        try:
            stream, segs = J.jpeg_scan_reference(data)
            padded = stream.tobytes() + bytes(-len(stream) % 8)
            want = "0 %d %d %d %d" % (len(stream), len(segs), zlib.adler32(padded), zlib.adler32(segs.tobytes()))
        except J.JpegRefused as e:
            want = "%d 0 0 0 0" % e.status
        assert line == want, name
    three = [tmp_path / (n + ".jpg") for n in ("8x8_noise_q85_s0", "rst1_grey", "17x33_grad_q30_s2")]
    run = subprocess.run([exe, "--truncations"] + [str(p) for p in three], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and run.stderr.strip() == "", run.stderr[-2000:]
    assert run.stdout.split("\n")[1::2][:3] == ["prefixes %d refused %d" % (os.path.getsize(p), os.path.getsize(p)) for p in three]
