"""Frozen model files without a GPU (include/ivit_modelfile.h, ivit_amd/model_file.py): the eighth header declares nine entries under
version 1 beside seven unchanged headers and the binding follows it; freeze_to_file / write / read round-trip five models byte for
byte and the format is pinned by two committed files; `ivit_model_file_info` (host only) agrees with `read`; the checksum has the
properties the format relies on; every corrupted variant of a file is refused by `read` and by the C reader with the same status and
the same text; and the C validator runs clean over all of them as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes
import hashlib
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden_scales, load_golden
import ivit_amd as iv
from ivit_amd import _abi, _lib, model_file as mf

ENTRIES = {"ivit_model_file_info": 4, "ivit_model_open": 4, "ivit_model_open_memory": 5, "ivit_model_get_info": 2, "ivit_model_vit": 2,
           "ivit_model_swin": 2, "ivit_model_constant": 4, "ivit_model_close": 1, "ivit_constants_checksum": 4}
MODELS = ["micro_vit_b2", "micro_vit2h_b3", "micro_swin_b2", "micro_swin_w12_b2", "deit_tiny_b1"]
INVALID, UNSUPPORTED = _lib.IVIT_ERR_INVALID, _lib.IVIT_ERR_UNSUPPORTED


# ---------------------------------------------------------------- the eighth header and its binding
def test_modelfile_header_declares_entries_and_version():
    hdr = open(os.path.join(ROOT, "include", "ivit_modelfile.h")).read()
    assert re.search(r'#include "ivit\.h"', hdr)
    assert int(re.search(r"#define IVIT_MODELFILE_VERSION (\d+)", hdr).group(1)) == 1 == _lib.IVIT_MODELFILE_VERSION
    assert _abi.MODELFILE_ABI.constants == {"IVIT_MODELFILE_VERSION": 1}
    assert list(_abi.MODELFILE_ABI.functions) == list(ENTRIES)
    assert "ivit_model" in _abi.MODELFILE_ABI.handles and "ivit_model" not in _abi.ABI.handles
    assert [d.name for d in _abi.MODELFILE_ABI.structs["ivit_model_info"]] == [
        "format", "kind", "img_size", "in_chans", "num_classes", "num_features", "records", "scalars", "file_bytes", "blob_bytes", "s_input",
        "s_features"]
    for name in ENTRIES:                                  # one "Alignment:" and one "Overlap:" line in front of every entry
        m = re.search(r"\bint %s\(" % name, hdr)
        front = hdr[hdr.rfind(";", 0, m.start()) + 1:m.start()]
        assert len(re.findall(r"\bAlignment:", front)) == 1 and len(re.findall(r"\bOverlap:", front)) == 1, name
    with pytest.raises(_abi.AbiError):                    # it names handles of ivit.h: it parses only with ivit.h as its base
        _abi.parse(hdr)


# the seven older headers: prototype count, version and sha256 of their prototypes (names, parameter types and names, in order).  The
# first six digests are those test_search_cpu.py pins; ivit_search.h's was computed with the same function on the parent commit
OLDER_HEADERS = {"ivit.h": (99, 111, "6817c4e822691347e82f51942395393d315550b28b44df8fd32f8d739abd6b52"),
                 "ivit_eval.h": (5, 1, "b47eee22a4d967fa3efca30b6994987eecccbe61cf040a3608941660bf3bee07"),
                 "ivit_features.h": (5, 1, "cb523d76e256d935c2b277e969372ad9fbcde8cbdb97559fa7d84a6516f2159f"),
                 "ivit_attnmap.h": (4, 1, "2f429e1f49a79e9a910707d666d5d274831c1f49f0e8177fd51abf43952572f6"),
                 "ivit_classmap.h": (3, 1, "8da355354133cbf09e4e986c0bb6e4081b79ba6c60ac3fdb746cceec64bc3620"),
                 "ivit_hidden.h": (7, 1, "e32b2dd1cfd7fa95a32729c1e3b888b5f32d46680928bf55b727671ba8d2f93f"),
                 "ivit_search.h": (4, 1, "9eb19bc2c54d09c40ef4eee451c7ed84db075aa304ded29c967e5abbfc9c57cb")}


def _prototypes_digest(abi):
    text = "\n".join(name + "(" + ", ".join(re.sub(r"\s+", " ", d.type) + " " + d.name for d in f.params) + ")"
                     for name, f in abi.functions.items())
    return hashlib.sha256(text.encode()).hexdigest()


def test_modelfile_entries_bound_and_exported_beside_unchanged_headers():
    iv.build()
    lib = _lib.load()
    P, I, Z = _lib._P, _lib._I, ctypes.c_size_t
    assert list(_lib.MODELFILE_SIGNATURES) == list(ENTRIES) == list(_lib.MODELFILE_RESTYPES)
    for name, nparams in ENTRIES.items():             # every bound name is exported, with the header's parameter count
        bound = getattr(lib, name)
        assert len(_lib.MODELFILE_SIGNATURES[name]) == nparams and bound.argtypes == _lib.MODELFILE_SIGNATURES[name] and bound.restype is I, name
    # the mapping rule: `const char *` and `const void **` parameters are c_void_p, size_t is c_size_t
    assert _lib.MODELFILE_SIGNATURES["ivit_model_file_info"] == [P, P, P, Z]
    assert _lib.MODELFILE_SIGNATURES["ivit_model_open"] == [P, P, I, P]
    assert _lib.MODELFILE_SIGNATURES["ivit_model_open_memory"] == [P, P, Z, I, P]
    assert _lib.MODELFILE_SIGNATURES["ivit_model_get_info"] == _lib.MODELFILE_SIGNATURES["ivit_model_vit"] == [P, P]
    assert _lib.MODELFILE_SIGNATURES["ivit_model_swin"] == [P, P] and _lib.MODELFILE_SIGNATURES["ivit_model_close"] == [P]
    assert _lib.MODELFILE_SIGNATURES["ivit_model_constant"] == [P, P, P, P]
    assert _lib.MODELFILE_SIGNATURES["ivit_constants_checksum"] == [P, P, Z, P]
    info = dict(_lib.ModelInfo._fields_)
    assert info["format"] is I and info["file_bytes"] is ctypes.c_int64 and info["s_input"] is ctypes.c_float and len(info) == 12
    versions = (_lib.IVIT_VERSION, _lib.IVIT_EVAL_VERSION, _lib.IVIT_FEATURES_VERSION, _lib.IVIT_ATTNMAP_VERSION, _lib.IVIT_CLASSMAP_VERSION,
                _lib.IVIT_HIDDEN_VERSION, _lib.IVIT_SEARCH_VERSION)
    abis = (_lib.ABI, _lib.EVAL_ABI, _lib.FEATURES_ABI, _lib.ATTNMAP_ABI, _lib.CLASSMAP_ABI, _lib.HIDDEN_ABI, _lib.SEARCH_ABI)
    older = set()
    for (name, (count, version, digest)), abi, v in zip(OLDER_HEADERS.items(), abis, versions):
        assert len(abi.functions) == count and v == version and _prototypes_digest(abi) == digest, name
        text = open(os.path.join(ROOT, "include", name)).read()
        assert _prototypes_digest(_abi.parse(text) if name == "ivit.h" else _abi.parse(text, base=_lib.ABI)) == digest, name
        assert "ivit_model_" not in text and "ivit_constants_checksum" not in text, name
        older |= set(abi.functions)
    assert not set(ENTRIES) & older


def test_build_follows_the_modelfile_header():
    so = iv.build()
    assert os.path.getmtime(so) >= os.path.getmtime(_abi.MODELFILE_HEADER)
    assert "ivit_modelfile.h" in _lib.SOURCES and os.path.exists(os.path.join(ROOT, "i-vit_amd", "csrc", "ivit_modelfile.h"))
    src = open(os.path.join(ROOT, "i-vit_amd", "_lib.py")).read()
    assert re.search(r"newest = max\(.*_abi\.HIDDEN_HEADER, _abi\.SEARCH_HEADER, _abi\.MODELFILE_HEADER", src)


def test_engines_and_tools_take_a_model_file():
    import inspect
    from ivit_amd.engine import ViTEngine
    from ivit_amd.native import NativeEngine
    from ivit_amd.swin_engine import SwinEngine
    for cls in (NativeEngine, ViTEngine, SwinEngine):
        assert list(inspect.signature(cls.save).parameters) == ["self", "path"] and callable(cls.input_scale_host), cls
    assert inspect.signature(ViTEngine.__init__).parameters["input_scale"].default is None          # optional keywords: no signature changed
    assert list(inspect.signature(ViTEngine.__init__).parameters)[:7] == ["self", "cfg", "consts", "f32", "device", "blob", "table"]
    assert list(inspect.signature(SwinEngine.__init__).parameters)[:7] == ["self", "cfg", "weights", "scales", "device", "packed", "exp_tables"]
    assert list(inspect.signature(mf.load_engine).parameters) == ["path", "device"] and iv.load_engine is mf.load_engine
    assert list(inspect.signature(mf.write).parameters) == ["path", "kind", "cfg", "blob", "table", "scalars", "extras"]
    assert list(inspect.signature(mf.freeze_to_file).parameters) == ["cfg", "weights", "scales", "path"]
    assert 'add_argument("--model-file"' in open(os.path.join(ROOT, "tools", "evaluate.py")).read()     # the helper the other tools import
    assert 'add_argument("--out"' in open(os.path.join(ROOT, "tools", "freeze.py")).read()


# ---------------------------------------------------------------- round trip and format pin
def _float_model(name):
    g = load_golden(name + ".npz")
    cname = str(g["cfg_name"])
    swin = cname in iv.SWIN_CONFIGS
    cfg = (iv.SWIN_CONFIGS if swin else iv.CONFIGS)[cname]
    return g, cfg, (iv.make_swin_weights if swin else iv.make_vit_weights)(cfg, int(g["seed"])), golden_scales(g)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (path of the file freeze_to_file wrote, its bytes, the golden, the package it was written from); built once"""
    d = tmp_path_factory.mktemp("modelfiles")
    out = {}
    for name in MODELS:
        g, cfg, w, s = _float_model(name)
        path = str(d / (name + ".ivit"))
        assert mf.freeze_to_file(cfg, w, s, path) == path
        out[name] = (path, open(path, "rb").read(), g, mf.frozen_package(cfg, w, s))
    return out


def _same_package(a, b):
    (kind, cfg, blob, table, scalars, extras), (kind2, cfg2, blob2, table2, scalars2, extras2) = a, b
    assert kind == kind2 and cfg == cfg2 and type(cfg) is type(cfg2)
    assert blob.dtype == blob2.dtype == np.uint8 and np.array_equal(blob, blob2)
    assert table == table2 and scalars == scalars2
    assert set(extras) == set(extras2)
    for k in extras:
        assert extras[k].dtype == extras2[k].dtype and extras[k].shape == extras2[k].shape and np.array_equal(extras[k], extras2[k]), k


@pytest.mark.parametrize("name", MODELS)
def test_read_of_write_is_the_package_and_writing_twice_gives_the_same_bytes(files, name, tmp_path):
    path, data, g, package = files[name]
    got = mf.read(path)
    _same_package(got, package)
    assert got[4]["input.s"] == ("f", float(g["scale/qact_input"]))
    kind = got[0]
    assert got[4]["feat.s"] == ("f", float(g["scale/qact2" if kind == "vit" else "scale/qact3"]))
    assert (sorted(got[5]) == ["class_scale"]) == (kind == "swin") and (kind == "swin" or not got[5])
    # every record keeps the offset pack_constants gives it
    from ivit_amd.engine import pack_constants
    if kind == "vit":
        from ivit_amd.engine import frozen_vit
        blob, table = pack_constants(frozen_vit(package[1], *_float_model(name)[2:])[0])
        assert table == got[3] and np.array_equal(blob, got[2])
    again = str(tmp_path / "again.ivit")
    mf.write(again, *package)
    assert open(again, "rb").read() == data == mf.to_bytes(*package) == mf.to_bytes(*got)
    # the layout the header states: blob at a 256-byte-aligned offset behind the tables, sizes that add up
    fmt, code, file_bytes, header_bytes, blob_offset, blob_bytes, core, nrec, nsca = struct.unpack_from("<II5QII", data, 8)
    assert data[:8] == b"IVITMDL\0" and fmt == 1 and code == (1 if kind == "vit" else 2) and file_bytes == len(data)
    assert header_bytes == 256 + 96 * nrec + 72 * nsca and blob_offset == -(-header_bytes // 256) * 256 and blob_offset + blob_bytes == len(data)
    assert core == got[2].size and nrec == len(got[3]) + len(got[5]) and nsca == len(got[4])
    assert max(len(k) for k in list(got[3]) + list(got[4])) < 48


PINNED = {"micro_vit_b2": "8dee6d922bb0b677fb5af43c0cd435e6f8fe49d671a5019a1c4b52efcb986ada",
          "micro_swin_b2": "fcfeedac56464d54dbdd962c3764668fa06cda3a37babb3e4f33d4c1f4dc184b"}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_format_version_1_is_pinned(files, name):
    """the sha256 of two files pins format version 1; both are under 1 MB and committed, so a file written today keeps loading"""
    path, data, g, package = files[name]
    assert hashlib.sha256(data).hexdigest() == PINNED[name]
    committed = os.path.join(GOLDEN, name + ".ivit")
    assert os.path.getsize(committed) < 1 << 20 and open(committed, "rb").read() == data
    _same_package(mf.read(committed), package)


# ---------------------------------------------------------------- ivit_model_file_info agrees with read
def _file_info(path):
    iv.build()
    lib = _lib.load()
    info, msg = _lib.ModelInfo(), ctypes.create_string_buffer(256)
    st = lib.ivit_model_file_info(os.fsencode(path), ctypes.byref(info), msg, len(msg))
    return st, msg.value.decode(), info


@pytest.mark.parametrize("name", MODELS)
def test_file_info_agrees_with_read(files, name):
    path, data, g, _ = files[name]
    kind, cfg, blob, table, scalars, extras = mf.read(path)
    st, msg, info = _file_info(path)
    assert st == _lib.IVIT_OK and msg == ""
    assert (info.format, info.kind) == (1, 1 if kind == "vit" else 2)
    assert (info.img_size, info.in_chans, info.num_classes) == (cfg.img_size, cfg.in_chans, cfg.num_classes)
    assert info.num_features == (cfg.embed_dim if kind == "vit" else cfg.num_features)
    assert (info.records, info.scalars) == (len(table) + len(extras), len(scalars))
    extra_bytes = sum(-(-a.nbytes // 256) * 256 for a in extras.values())
    assert info.file_bytes == len(data) and info.blob_bytes == blob.size + extra_bytes
    assert np.float32(info.s_input) == np.float32(scalars["input.s"][1]) == g["scale/qact_input"]
    assert np.float32(info.s_features) == np.float32(scalars["feat.s"][1])


# ---------------------------------------------------------------- the checksum
def _mix(z):
    z &= 2 ** 64 - 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
    return z ^ (z >> 31)


def _checksum_by_hand(data):
    data = bytes(data) + b"\0" * (-len(data) % 8)
    return sum(_mix(int.from_bytes(data[8 * i:8 * i + 8], "little") ^ ((i + 1) * 0x9E3779B97F4A7C15)) for i in range(len(data) // 8)) % 2 ** 64


def test_checksum_reference_properties():
    """sizes around a word; every single-bit flip and a swap of two different words change the sum.  A zero byte appended inside the
    same word does NOT change it: the tail is zero-padded — harmless, the file stores every length (a longer file is refused by its
    size fields before a checksum is looked at)."""
    rng = np.random.default_rng(3)
    for n in (0, 1, 7, 8, 9, 4099):
        data = rng.integers(0, 256, n, dtype=np.uint8)
        assert mf.checksum_reference(data) == mf.checksum_reference(data.tobytes()) == _checksum_by_hand(data.tobytes()), n
    assert mf.checksum_reference(b"") == 0
    buf = rng.integers(0, 256, 64, dtype=np.uint8)
    base = mf.checksum_reference(buf)
    seen = {base}
    for bit in range(64 * 8):
        flipped = buf.copy()
        flipped[bit // 8] ^= 1 << (bit % 8)
        seen.add(mf.checksum_reference(flipped))
    assert len(seen) == 64 * 8 + 1                        # all different from the original, and from each other
    words = buf.view("<u8").copy()
    assert words[1] != words[5]
    words[[1, 5]] = words[[5, 1]]
    assert mf.checksum_reference(words.view(np.uint8)) != base
    assert mf.checksum_reference(bytes(buf[:13]) + b"\0") == mf.checksum_reference(buf[:13])            # same word: same sum
    assert mf.checksum_reference(bytes(buf[:16]) + b"\0") != mf.checksum_reference(buf[:16])            # a new word: another sum
    # the header's own field is left out by taking its word as zero
    zeroed = buf.copy()
    zeroed[8:16] = 0
    assert mf.checksum_reference(buf, skip=8) == mf.checksum_reference(zeroed)


# ---------------------------------------------------------------- refusals
def _reseal(data):
    """both checksums recomputed: a variant then reaches the check it is about, not the checksum in front of it"""
    data = bytearray(data)
    blob_offset = struct.unpack_from("<Q", data, 32)[0]
    if 256 <= blob_offset <= len(data):
        struct.pack_into("<Q", data, 72, mf.checksum_reference(bytes(data[blob_offset:])))
        struct.pack_into("<Q", data, 64, mf.checksum_reference(bytes(data[:blob_offset]), skip=64))
    return bytes(data)


def _patched(data, offset, fmt, *values, reseal=True):
    data = bytearray(data)
    struct.pack_into(fmt, data, offset, *values)
    return _reseal(data) if reseal else bytes(data)


def _record_offset(data, name):
    nrec = struct.unpack_from("<I", data, 56)[0]
    for i in range(nrec):
        p = 256 + 96 * i
        if data[p:p + 48].split(b"\0")[0] == name.encode():
            return p
    raise KeyError(name)


def _variants(data, package):
    """(id, bytes, status, what the message names) for every corrupted form of the micro_vit_b2 file"""
    kind, cfg, blob, table, scalars, extras = package
    nrec, nsca = struct.unpack_from("<II", data, 56)
    header_bytes, blob_offset = struct.unpack_from("<QQ", data, 24)
    blob_bytes = len(data) - blob_offset
    out = []
    # truncated at each section boundary and one byte either side (the file's end + 1: one byte too many)
    for what, b in (("fixed", 256), ("records", 256 + 96 * nrec), ("scalars", header_bytes), ("blob", blob_offset), ("end", len(data))):
        for cut in (b - 1, b, b + 1):
            if cut != len(data):
                out.append((f"cut-{what}-{cut - b:+d}", (data + b"\0")[:cut], INVALID, "header: file holds %d bytes" % cut))
    out.append(("size-field", _patched(data, 16, "<Q", len(data) + 256), INVALID, "its header says %d" % (len(data) + 256)))
    flipped = bytearray(data)
    flipped[150] ^= 0x10
    out.append(("bit-in-header", bytes(flipped), INVALID, "header: checksum"))
    flipped = bytearray(data)
    flipped[blob_offset + 1000] ^= 0x01
    out.append(("bit-in-blob", bytes(flipped), INVALID, "blob: checksum"))
    out.append(("version-2", _patched(data, 8, "<I", 2), UNSUPPORTED, "format version 2 is newer"))
    out.append(("kind-3", _patched(data, 12, "<I", 3), UNSUPPORTED, "unknown kind 3"))
    out.append(("record-count", _patched(data, 56, "<I", 2 ** 31 - 1), INVALID, "records: count 2147483647 exceeds"))
    r0, r1 = 256, 256 + 96
    name0, name1 = (data[p:p + 48].split(b"\0")[0].decode() for p in (r0, r1))
    off0 = struct.unpack_from("<Q", data, r0 + 80)[0]
    out.append(("record-past-blob", _patched(data, r1 + 80, "<Q", blob_bytes), INVALID, f'"{name1}": offset {blob_bytes} + '))
    out.append(("records-overlap", _patched(data, r1 + 80, "<Q", off0), INVALID, f'records "{name0}" and "{name1}" overlap'))
    out.append(("odd-offset", _patched(data, r1 + 80, "<Q", struct.unpack_from("<Q", data, r1 + 80)[0] + 1), INVALID, "is not a multiple of 256"))
    out.append(("name-unterminated", _patched(data, r1, "48s", b"b" * 48), INVALID, "record 1: name is empty or not terminated"))
    out.append(("name-duplicate", _patched(data, r1, "48s", name0.encode()), INVALID, f'record 1 "{name0}": duplicate name'))
    out.append(("dtype-unknown", _patched(data, r1 + 48, "<I", 9), INVALID, "unknown dtype code 9"))
    # records removed or reshaped: the file is written again from an edited table (the blob keeps its bytes)
    without = lambda *names: {k: v for k, v in table.items() if k not in names}      # noqa: E731
    out.append(("no-head.w", mf.to_bytes(kind, cfg, blob, without("head.w"), scalars, extras), INVALID, 'record "head.w" is missing'))
    o, dt, (n, k) = table["blocks.0.attn.qkv.w"]
    D = cfg.embed_dim
    assert (n, k) == (3 * D, D)
    out.append(("qkv-transposed", mf.to_bytes(kind, cfg, blob, dict(table, **{"blocks.0.attn.qkv.w": (o, dt, (k, n))}), scalars, extras), INVALID,
                f'record "blocks.0.attn.qkv.w" is i1 [{D}, {3 * D}, 0], the configuration implies i1 [{3 * D}, {D}, 0]'))
    tabled = [i for i in range(cfg.depth) if f"blocks.{i}.attn.exp_t" in table]
    assert tabled, "the fixture has a block with Shiftmax tables"
    out.append(("shiftmax-partly", mf.to_bytes(kind, cfg, blob, without(f"blocks.{tabled[0]}.attn.exp_t"), scalars, extras), INVALID,
                f'Shiftmax tables of "blocks.{tabled[0]}.attn" are partly present (3 of 4 records)'))
    out.append(("depth-0", _patched(data, 80 + 4 * 4, "<i", 0), INVALID, "config: depth 0 is outside 1 .. 4096"))
    out.append(("depth-1e9", _patched(data, 80 + 4 * 4, "<i", 10 ** 9), INVALID, "config: depth 1000000000 is outside 1 .. 4096"))
    assert len({v[0] for v in out}) == len(out)
    return out


@pytest.fixture(scope="module")
def variants(files, tmp_path_factory):
    """[(id, path, bytes, status, text)], the good file first (status 0)"""
    path, data, g, package = files["micro_vit_b2"]
    d = tmp_path_factory.mktemp("variants")
    out = [("good", path, data, _lib.IVIT_OK, "")]
    for vid, b, status, text in _variants(data, package):
        p = str(d / (vid + ".ivit"))
        with open(p, "wb") as f:
            f.write(b)
        out.append((vid, p, b, status, text))
    return out


def test_every_corrupted_variant_is_refused_by_read_and_by_the_c_reader_alike(variants):
    assert len(variants) == 1 + 14 + 17
    for vid, path, data, status, text in variants:
        st, msg, info = _file_info(path)
        if status == _lib.IVIT_OK:
            mf.read_bytes(data)
            assert st == _lib.IVIT_OK and msg == "" and info.records > 0, vid
            continue
        with pytest.raises(mf.ModelFileError) as e:
            mf.read_bytes(data)
        assert e.value.status == status and text in str(e.value), (vid, str(e.value))
        assert st == status and msg == str(e.value), (vid, msg, str(e.value))        # the same status, the same wording
        assert info.records == 0 and info.file_bytes == 0, vid
    st, msg, _ = _file_info(os.path.join(os.path.dirname(variants[0][1]), "no-such-file.ivit"))
    assert st == INVALID and msg.startswith("file: cannot open")
    with pytest.raises(mf.ModelFileError, match="file: cannot open"):
        mf.read(os.path.join(os.path.dirname(variants[0][1]), "no-such-file.ivit"))


# ---------------------------------------------------------------- the validator under sanitizers, as a stand-alone program
SANITIZE = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"]


def test_validator_runs_clean_under_sanitizers(variants, tmp_path):
    """tests/modelfile_harness.cpp — its own main, the host half of csrc/ivit_modelfile.h — built with the host compiler and
    -fsanitize=address,undefined, run over the good file and every corrupted variant: exit status 0, nothing from a sanitizer on
    stderr, the statuses of the test above.  Nothing is preloaded and nothing is loaded into Python.  Leak detection is off (it
    needs ptrace, which a sandboxed runner may lack); the memory and undefined-behaviour checks are what a hostile file can reach.
    Skips only where a one-line sanitised program does not build."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if not cxx or subprocess.run([cxx] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no host compiler builds a sanitised program here")
    exe = str(tmp_path / "modelfile_harness")
    subprocess.run([cxx] + SANITIZE + [os.path.join(ROOT, "tests", "modelfile_harness.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    paths = [v[1] for v in variants] + [str(tmp_path / "no-such-file.ivit")]
    run = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, run.stderr[-2000:]
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr and run.stderr.strip() == "", run.stderr[-2000:]
    lines = run.stdout.strip().split("\n")
    assert len(lines) == len(paths)
    for (vid, _, _, status, text), line in zip(variants, lines):
        st, msg = line.split("\t", 1)
        assert int(st) == status and (text in msg if status else msg.startswith("ok kind 1 records")), (vid, line)
    assert lines[-1].startswith(f"{INVALID}\tfile: cannot open")


# ---------------------------------------------------------------- the kernel in the code object
def test_checksum_kernel_in_code_object_without_scratch(tmp_path):
    """the one new kernel: in the gfx950 code object, no scratch, no spills, 32 bytes of LDS (four 64-bit partial sums)"""
    from test_cabi_cpu import _device_code_object
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        readelf = shutil.which("llvm-readelf")
    assert readelf, "llvm-readelf not found"
    co = tmp_path / "dev.co"
    co.write_bytes(_device_code_object(iv.build()))
    notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True, check=True).stdout
    found = []
    for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        if nm and re.fullmatch(r"_Z\d+constants_checksum_kernel\w+", nm.group(1)):
            found.append(tuple(int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
                               for key in ("private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size")))
    assert found == [(0, 0, 32)], found
