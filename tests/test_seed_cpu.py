"""k-means++ seeding without a GPU: include/ivit_seed.h declares two entries under version 1, the binding follows it, the numpy statement
on a hand-computable case and with fewer distinct rows than K, and the kernels in the gfx950 code object."""
import os
import re
import shutil
import subprocess

import numpy as np

from conftest import ROOT
import ivit_amd as iv
from ivit_amd import _abi, _lib
from ivit_amd.predict import kmeans_seed_reference

ENTRIES = {"ivit_kmeans_seed_workspace_bytes": 4, "ivit_kmeans_seed": 15}


def test_seed_header_declares_entries_under_version_1():
    hdr = open(_abi.SEED_HEADER).read()
    assert re.search(r'#include "ivit\.h"', hdr)
    assert int(re.search(r"#define IVIT_SEED_VERSION (\d+)", hdr).group(1)) == 1 == _lib.IVIT_SEED_VERSION
    assert _abi.SEED_ABI.constants == {"IVIT_SEED_VERSION": 1} and list(_abi.SEED_ABI.functions) == list(ENTRIES)
    for name in ENTRIES:                                  # one "Alignment:" and one "Overlap:" line in front of every entry
        m = re.search(r"\bint %s\(" % name, hdr)
        front = hdr[hdr.rfind(";", 0, m.start()) + 1:m.start()]
        assert len(re.findall(r"\bAlignment:", front)) == 1 and len(re.findall(r"\bOverlap:", front)) == 1, name
    assert [p.name for p in _abi.SEED_ABI.functions["ivit_kmeans_seed"].params] == [
        "h", "x", "rows", "dim", "K", "trials", "first", "draws", "workspace", "workspace_bytes", "cent", "cnorm", "idx", "potential", "picked"]


def test_seed_entries_bound_exported_and_built():
    so = iv.build()
    lib = _lib.load()
    assert list(_lib.SEED_SIGNATURES) == list(ENTRIES) == list(_lib.SEED_RESTYPES)
    for name, nparams in ENTRIES.items():                 # every bound name is exported, with the header's parameter count
        bound = getattr(lib, name)
        assert len(_lib.SEED_SIGNATURES[name]) == nparams and bound.argtypes == _lib.SEED_SIGNATURES[name] and bound.restype is _lib._I, name
    assert os.path.getmtime(so) >= os.path.getmtime(_abi.SEED_HEADER) and "ivit_seed.h" in _lib.SOURCES
    assert re.search(r"newest = max\(.*_abi\.JPEG_ENTROPY_HEADER, _abi\.SEED_HEADER", open(os.path.join(ROOT, "i-vit_amd", "_lib.py")).read())


def _unit(cols):
    """a dim-64 row that holds 1 in the given number of leading columns: d(unit(a), unit(b)) = |a - b|"""
    r = np.zeros(64, np.int8)
    r[:cols] = 1
    return r


def test_reference_on_a_hand_case():
    # rows at positions 0, 0, 1, 3, 7, 16 on a line (squared distance = difference); first = row 0: mind = [0, 0, 1, 3, 7, 16], total 27,
    # cumsum = [0, 0, 1, 4, 11, 27]
    x = np.stack([_unit(c) for c in (0, 0, 1, 3, 7, 16)])
    draw = lambda t, total: np.uint64(-(-(t << 64) // total))          # the smallest draw with (draw * total) >> 64 == t
    d = np.zeros((3, 2), np.uint64)
    # step 1: t = 0 skips both zero rows and lands on row 2 (side="right"); t = 10 is the last unit of row 4 (cumsum 11 > 10)
    d[1] = draw(0, 27), draw(10, 27)
    idx, cent, cnorm, pot, picked = kmeans_seed_reference(x, 3, 0, d)
    # candidates: row 2 -> min(mind, |p - 1|) = [0,0,0,2,6,15] = 23; row 4 -> [0,0,1,3,0,9] = 13: the second wins
    assert idx[1] == 4 and pot.tolist()[:2] == [27, 13]
    d[1] = draw(10, 27), draw(11, 27)                     # t = 11 is the first unit of row 5: [0,0,1,3,7,0] = 11 beats 13
    d[2] = draw(3, 11), draw(3, 11)                       # equal candidates (row 3: cumsum [0,0,1,4,..] > 3): the lower l, same row
    idx, cent, cnorm, pot, picked = kmeans_seed_reference(x, 3, 0, d)
    assert idx.tolist() == [0, 5, 3] and pot.tolist() == [27, 11, 5] and picked.tolist() == [3]
    assert idx.dtype == np.int32 and pot.dtype == np.int64 and np.array_equal(cent, x[[0, 5, 3]]) and cnorm.tolist() == [0, 16, 3]
    d[1] = np.uint64(2 ** 64 - 1)                         # the largest draw stays below the total: the last row, never past the end
    assert kmeans_seed_reference(x, 3, 0, d)[0][1] == 5


def test_reference_with_fewer_distinct_rows_than_K():
    rng = np.random.default_rng(0)
    x = np.repeat(rng.integers(-128, 128, size=(5, 64)).astype(np.int8), 4, axis=0)
    idx, cent, cnorm, pot, picked = kmeans_seed_reference(x, 8, 3, rng.integers(0, 2 ** 64, size=(8, 3), dtype=np.uint64))
    assert picked.tolist() == [5] and (idx[5:] == -1).all() and pot[4] == 0 and (pot[:4] > 0).all() and (pot[5:] == 0).all()
    assert len(np.unique(x[idx[:5]], axis=0)) == 5 and (np.diff(pot[:5]) <= 0).all()


def test_seed_kernels_in_code_object_without_scratch(tmp_path):
    from test_cabi_cpu import _device_code_object
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        readelf = shutil.which("llvm-readelf")
    assert readelf, "llvm-readelf not found"
    co = tmp_path / "dev.co"
    co.write_bytes(_device_code_object(iv.build()))
    notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True, check=True).stdout
    scratch = {m.group(1): int(m.group(2)) for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]
               for m in [re.search(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)", blk, re.S)] if m}
    scans = [k for k in scratch if re.fullmatch(r"_Z\d+seed_scan_kernelILi\d+ELb[01]EE\w+", k)]
    assert len(scans) == 16 and sum("ELb1E" in k for k in scans) == 7          # dim 64 .. 1024, prefetching up to 448
    for k in scans + [next(k for k in scratch if name in k) for name in ("seed_setup_kernel", "seed_pick_kernel", "seed_locate_kernel")]:
        assert scratch[k] == 0, k
