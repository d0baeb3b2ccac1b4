"""Frozen model files on the device (include/ivit_modelfile.h).  The Python path: an engine loaded from the file its original saved
gives the original's tensors bit for bit on every entry, the golden logits, the input scale and — a Swin — the class maps' unit, and
saves the same bytes again.  The C path through ctypes: ivit_model_open -> the borrowed runner -> workspace -> forward gives the golden
logits with one and two slices, from a path and from memory; a corrupted file is refused with *out NULL.  ivit_constants_checksum
equals `checksum_reference` at every size around a piece, a word and a grid pass, reads nothing beyond `bytes`, replays in a graph and
verifies an uploaded blob.  The built example classifies the golden images in a process without Python, and the tools take
--model-file."""
import ctypes
import importlib.util
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden_scales, load_golden
import ivit_amd as iv
from ivit_amd import _lib, model_file as mf

pytestmark = pytest.mark.gpu
_P = ctypes.c_void_p
MODELS = ["micro_vit_b2", "micro_vit2h_b3", "micro_swin_b2", "micro_swin_w12_b2", "deit_tiny_b1"]


def P(t, offset=0):
    return _P(t.data_ptr() + offset)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def flat(out):
    """the tensors of a result, nested tuples opened, None dropped"""
    if out is None:
        return []
    if isinstance(out, tuple):
        return [t for o in out for t in flat(o)]
    return [out]


def same(a, b):
    a, b = flat(a), flat(b)
    assert len(a) == len(b) and len(a) > 0
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.data_ptr() != y.data_ptr()
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))       # bit for bit, NaN and -0.0 included


_CACHE = {}


def model(name, tmp_root):
    """(golden, cfg, the engine built from float weights, the file it saved, the engine loaded from it), built once per model"""
    if name not in _CACHE:
        g = load_golden(name + ".npz")
        cname = str(g["cfg_name"])
        if cname in iv.SWIN_CONFIGS:
            from ivit_amd.swin_engine import SwinEngine
            cfg = iv.SWIN_CONFIGS[cname]
            weights = iv.make_swin_weights(cfg, int(g["seed"]))
            eng = SwinEngine(cfg, weights, golden_scales(g))
        else:
            from ivit_amd.engine import ViTEngine
            cfg = iv.CONFIGS[cname]
            weights = iv.make_vit_weights(cfg, int(g["seed"]))
            eng = ViTEngine.from_float(cfg, weights, golden_scales(g))
        path = str(tmp_root / (name + ".ivit"))
        assert eng.save(path) == path
        frozen = str(tmp_root / (name + ".frozen.ivit"))                 # the host-only route gives the same bytes as the device's blob
        mf.freeze_to_file(cfg, weights, golden_scales(g), frozen)
        assert open(frozen, "rb").read() == open(path, "rb").read()
        _CACHE[name] = (g, cfg, eng, path, iv.load_engine(path))
    return _CACHE[name]


@pytest.fixture(scope="module")
def tmp_root(tmp_path_factory):
    yield tmp_path_factory.mktemp("modelfiles_gpu")
    _CACHE.clear()


def golden_images(g, cfg):
    return dev(iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"])))


# ---------------------------------------------------------------- the Python path
@pytest.mark.parametrize("name", MODELS)
def test_loaded_engine_is_the_engine_that_was_saved(name, tmp_root, tmp_path):
    g, cfg, eng, path, loaded = model(name, tmp_root)
    assert type(loaded) is type(eng) and loaded.cfg == cfg and loaded is not eng
    assert loaded.table == eng.table and torch.equal(loaded.blob, eng.blob) and loaded.blob.data_ptr() != eng.blob.data_ptr()
    imgs = golden_images(g, cfg)
    B = imgs.shape[0]
    assert np.array_equal(loaded.forward(imgs).cpu().numpy(), g["logits_int"])
    k = min(5, cfg.num_classes)
    same(loaded.predict(imgs, k=k, copy=True), eng.predict(imgs, k=k, copy=True))
    labels = (torch.arange(B, device="cuda", dtype=torch.int64) * 3 + 1) % cfg.num_classes
    same(loaded.score(imgs, labels, copy=True), eng.score(imgs, labels, copy=True))
    for unit in (False, True):
        same(loaded.features(imgs, normalize=unit, logits=True, copy=True), eng.features(imgs, normalize=unit, logits=True, copy=True))
    sites = (0, -1)
    same(loaded.hidden_states(imgs, sites, layout="tokens", logits=True, copy=True), eng.hidden_states(imgs, sites, layout="tokens", logits=True, copy=True))
    same(loaded.hidden_states(imgs, sites, layout="grid", copy=True), eng.hidden_states(imgs, sites, layout="grid", copy=True))
    for i in sites:
        assert loaded.hidden_scale_host(i) == eng.hidden_scale_host(i)
    if hasattr(eng, "attention"):
        same(loaded.attention(imgs, blocks=(0, -1), heads=True, logits=True, copy=True), eng.attention(imgs, blocks=(0, -1), heads=True, logits=True, copy=True))
        same(loaded.forward_ops(imgs).clone(), eng.forward_ops(imgs).clone())
        assert loaded.f32 == eng.f32
    else:
        assert torch.equal(loaded.class_scale, eng.class_scale) and loaded.class_scale.dtype == torch.float32        # from the file
        same(loaded.class_map(imgs, k=min(3, cfg.num_classes), copy=True), eng.class_map(imgs, k=min(3, cfg.num_classes), copy=True))
        same(loaded.forward_ops(imgs).clone(), eng.forward_ops(imgs).clone())
        assert loaded.host_consts == eng.host_consts
    same(loaded.capture_predict(imgs, k=k)(), eng.capture_predict(imgs, k=k)())
    assert np.array_equal(loaded.head_scale_host(), eng.head_scale_host()) and loaded.feature_scale_host() == eng.feature_scale_host()
    assert np.float32(loaded.input_scale_host()) == np.float32(eng.input_scale_host()) == g["scale/qact_input"]
    again = str(tmp_path / "again.ivit")
    loaded.save(again)
    assert open(again, "rb").read() == open(path, "rb").read()


def test_retrieve_on_a_loaded_engine(tmp_root):
    from ivit_amd.search import Gallery
    g, cfg, eng, path, loaded = model("micro_vit2h_b3", tmp_root)
    rows = dev(iv.make_images_int8(cfg, 9, seed=5))
    gallery = Gallery(eng.features(rows, copy=True)[0], cosine=True)
    imgs = golden_images(g, cfg)
    same(loaded.retrieve(imgs, gallery, k=4, copy=True), eng.retrieve(imgs, gallery, k=4, copy=True))


def test_an_engine_that_was_never_told_says_so(tmp_root, tmp_path):
    """a Swin built from a broadcast package (packed=) still has neither the input scale nor class_scale: the package carries what it
    carried; the optional keyword gives the input scale"""
    from ivit_amd.swin_engine import SwinEngine, packed_swin
    g, cfg, eng, path, loaded = model("micro_swin_b2", tmp_root)
    packed = packed_swin(cfg, iv.make_swin_weights(cfg, int(g["seed"])), golden_scales(g))
    bare = SwinEngine(cfg, None, None, packed=packed)
    with pytest.raises(_lib.IvitError, match="never told its input scale"):
        bare.input_scale_host()
    with pytest.raises(_lib.IvitError, match="class_scale"):
        bare.class_scale
    with pytest.raises(_lib.IvitError):
        bare.save(str(tmp_path / "bare.ivit"))
    told = SwinEngine(cfg, None, None, packed=packed, input_scale=g["scale/qact_input"])
    assert np.float32(told.input_scale_host()) == g["scale/qact_input"]
    assert np.array_equal(bare.forward(golden_images(g, cfg)).cpu().numpy(), g["logits_int"])


# ---------------------------------------------------------------- the C path through ctypes
def c_open(h, path=None, data=None, max_slices=2):
    m = _P()
    if data is None:
        st = h.lib.ivit_model_open(h.h, os.fsencode(path), max_slices, ctypes.byref(m))
    else:
        st = h.lib.ivit_model_open_memory(h.h, data, len(data), max_slices, ctypes.byref(m))
    return st, m


def c_forward(h, m, vit, imgs, num_classes, nslices):
    """ivit_model_vit / _swin -> ivit_*_workspace_bytes / _init -> ivit_*_forward, as a C host would"""
    lib, prefix, run, B = h.lib, "ivit_vit" if vit else "ivit_swin", _P(), imgs.shape[0]
    h._check(getattr(lib, "ivit_model_vit" if vit else "ivit_model_swin")(m, ctypes.byref(run)), "ivit_model_vit / _swin")
    n = ctypes.c_size_t()
    h._check(getattr(lib, prefix + "_workspace_bytes")(run, B, nslices, ctypes.byref(n)), prefix + "_workspace_bytes")
    ws = torch.empty(max(1, n.value), dtype=torch.uint8, device="cuda")
    logits = torch.full((B, num_classes), -7, dtype=torch.int32, device="cuda")
    if vit:
        h._check(lib.ivit_vit_workspace_init(run, P(ws), n.value, B, nslices), "ivit_vit_workspace_init")
    h._check(getattr(lib, prefix + "_forward")(run, P(imgs), B, nslices, P(ws), n.value, P(logits)), prefix + "_forward")
    torch.cuda.synchronize()
    return logits.cpu().numpy()


def device_bytes(ptr, n):
    """n bytes of device memory at a raw address (the HIP runtime the process already holds)"""
    out = np.empty(n, np.uint8)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes, hip.hipMemcpy.restype = [_P, _P, ctypes.c_size_t, ctypes.c_int], ctypes.c_int
    torch.cuda.synchronize()
    assert hip.hipMemcpy(_P(out.ctypes.data), ptr, n, 2) == 0                     # hipMemcpyDeviceToHost
    return out


@pytest.mark.parametrize("name", MODELS)
def test_c_host_opens_the_file_and_runs_the_golden_batch(name, tmp_root):
    g, cfg, eng, path, _ = model(name, tmp_root)
    vit = str(g["cfg_name"]) in iv.CONFIGS
    h = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    lib = h.lib
    imgs, want = golden_images(g, cfg), g["logits_int"]
    if imgs.shape[0] == 1:                                                          # two slices need two images: the golden image twice
        imgs, want = torch.cat([imgs, imgs]).contiguous(), np.concatenate([want, want])
    data = open(path, "rb").read()
    for source in ("path", "memory", "path"):                                       # ... and a fresh open after a close works
        st, m = c_open(h, path) if source == "path" else c_open(h, data=data)
        assert st == _lib.IVIT_OK and m.value, (source, lib.ivit_last_error(h.h))
        for nslices in (1, 2):
            assert np.array_equal(c_forward(h, m, vit, imgs, cfg.num_classes, nslices), want), (source, nslices)
        other = _P(1)
        assert getattr(lib, "ivit_model_swin" if vit else "ivit_model_vit")(m, ctypes.byref(other)) == _lib.IVIT_ERR_INVALID and not other.value
        info = _lib.ModelInfo()
        assert lib.ivit_model_get_info(m, ctypes.byref(info)) == _lib.IVIT_OK
        assert (info.kind, info.num_classes, info.file_bytes) == (1 if vit else 2, cfg.num_classes, len(data))
        assert np.float32(info.s_input) == g["scale/qact_input"] and np.float32(info.s_features) == np.float32(eng.feature_scale_host())
        ptr, n = _P(), ctypes.c_size_t()
        assert lib.ivit_model_constant(m, b"head.scale", ctypes.byref(ptr), ctypes.byref(n)) == _lib.IVIT_OK and n.value == 4 * cfg.num_classes
        assert np.array_equal(device_bytes(ptr, n.value).view(np.float32), eng.head_scale_host()) and ptr.value % 256 == 0
        if not vit:
            assert lib.ivit_model_constant(m, b"class_scale", ctypes.byref(ptr), ctypes.byref(n)) == _lib.IVIT_OK and n.value == 4 * cfg.num_classes
            assert np.array_equal(device_bytes(ptr, n.value).view(np.float32), eng.class_scale.cpu().numpy())
        assert lib.ivit_model_constant(m, b"no.such.record", ctypes.byref(ptr), ctypes.byref(n)) == _lib.IVIT_ERR_INVALID and not ptr.value
        assert b"no.such.record" in lib.ivit_last_error(h.h)
        assert lib.ivit_model_close(m) == _lib.IVIT_OK
    h.close()


def test_c_host_refuses_a_corrupted_file_and_frees_everything(tmp_root, tmp_path):
    g, cfg, eng, path, _ = model("micro_vit_b2", tmp_root)
    h = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    data = bytearray(open(path, "rb").read())
    blob_offset = struct.unpack_from("<Q", data, 32)[0]
    data[blob_offset + 1000] ^= 0x01
    st, m = c_open(h, data=bytes(data))
    assert st == _lib.IVIT_ERR_INVALID and not m.value and b"blob: checksum" in h.lib.ivit_last_error(h.h)
    newer = bytearray(open(path, "rb").read())
    struct.pack_into("<I", newer, 8, 2)
    st, m = c_open(h, data=bytes(newer))
    assert st == _lib.IVIT_ERR_UNSUPPORTED and not m.value and b"format version 2" in h.lib.ivit_last_error(h.h)
    st, m = c_open(h, str(tmp_path / "no-such-file.ivit"))
    assert st == _lib.IVIT_ERR_INVALID and not m.value and b"cannot open" in h.lib.ivit_last_error(h.h)
    st, m = c_open(h, path, max_slices=0)
    assert st == _lib.IVIT_ERR_INVALID and not m.value and b"max_slices" in h.lib.ivit_last_error(h.h)
    st, m = c_open(h, path)                                                         # the good file still opens
    assert st == _lib.IVIT_OK and m.value and h.lib.ivit_model_close(m) == _lib.IVIT_OK
    h.close()


# ---------------------------------------------------------------- ivit_constants_checksum
GUARD = 64


def device_checksum(h, buf, n):
    out = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    h.call("ivit_constants_checksum", P(buf), n, P(out))
    torch.cuda.synchronize()
    return int(out.cpu().numpy().view(np.uint64)[0])


# around a byte, a word (8), a piece (16), a workgroup's step (256 threads x 16 bytes = 4096), and 8 MiB + 5: more than one pass of the
# capped grid (4 workgroups per CU, 4 MiB a pass on 256 CUs) with a tail
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 15, 16, 17, 255, 256, 257, 4099, (8 << 20) + 5])
def test_checksum_equals_the_reference_and_reads_nothing_beyond_bytes(n):
    h = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(1000 + n % 997)
    data = rng.integers(0, 256, n, dtype=np.uint8)
    want = mf.checksum_reference(data)
    buf = torch.empty(n + GUARD, dtype=torch.uint8, device="cuda")
    buf[:n] = dev(data)
    for poison in (0xA5, 0x5A):                             # the guard behind the payload changes between the runs: the sum does not
        buf[n:] = poison
        assert device_checksum(h, buf, n) == want, (n, poison)
    assert np.array_equal(buf[:n].cpu().numpy(), data) and bool((buf[n:] == 0x5A).all())
    if n:
        st = h.lib.ivit_constants_checksum(h.h, P(buf, 8), n, P(torch.zeros(1, dtype=torch.int64, device="cuda")))
        assert st == _lib.IVIT_ERR_INVALID and b"16-byte aligned" in h.lib.ivit_last_error(h.h)
    h.close()


def _torch_checksum(buf, n):
    """the checksum of buf[:n] in torch int64 arithmetic on the device, chunk by chunk: a second statement of the definition that
    can be afforded at 4 GiB (int64 products and sums wrap mod 2^64; a logical shift is an arithmetic one with the sign bits masked)"""
    signed = lambda v: v - (1 << 64) if v >= 1 << 63 else v      # noqa: E731
    lsr = lambda z, s: (z >> s) & ((1 << (64 - s)) - 1)           # noqa: E731
    K, C1, C2 = signed(0x9E3779B97F4A7C15), signed(0xBF58476D1CE4E5B9), signed(0x94D049BB133111EB)
    words, total, chunk = n // 8, 0, 1 << 24
    w = buf[:words * 8].view(torch.int64)
    for start in range(0, words, chunk):
        x = w[start:start + chunk]
        z = x ^ (torch.arange(start + 1, start + 1 + x.numel(), device="cuda", dtype=torch.int64) * K)
        z = (z ^ lsr(z, 30)) * C1
        z = (z ^ lsr(z, 27)) * C2
        z = z ^ lsr(z, 31)
        total += int(z.sum().item())
    if n % 8:
        tail = int.from_bytes(bytes(buf[words * 8:n].cpu().numpy()), "little") ^ (((words + 1) * 0x9E3779B97F4A7C15) % 2 ** 64)
        tail = ((tail ^ (tail >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
        tail = ((tail ^ (tail >> 27)) * 0x94D049BB133111EB) % 2 ** 64
        total += tail ^ (tail >> 31)
    return total % 2 ** 64


def test_checksum_above_4_gib():
    """4 GiB + 21 bytes: piece indices past 2^28, byte offsets past 2^32, 1024 passes of the capped grid and a tail of two words.  The
    reference at this size is the torch statement above, itself held to `checksum_reference` at a size numpy affords"""
    n = (4 << 30) + 21
    free = torch.cuda.mem_get_info()[0]
    if free < 2 * n:
        pytest.skip(f"{free} bytes free on the device, {2 * n} needed")
    h = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    buf = torch.empty(n + GUARD, dtype=torch.uint8, device="cuda")
    buf[:n // 8 * 8].view(torch.int64).random_()
    buf[n // 8 * 8:] = 0xC3
    small = (1 << 20) + 13
    assert _torch_checksum(buf, small) == mf.checksum_reference(buf[:small].cpu().numpy()) == device_checksum(h, buf, small)
    want = _torch_checksum(buf, n)
    assert device_checksum(h, buf, n) == want
    buf[n - 1] ^= 0x80                                      # the last byte, behind 2^32, is part of the sum; the guard is not
    flipped = device_checksum(h, buf, n)
    assert flipped != want and flipped == _torch_checksum(buf, n)
    buf[n:] = 0x3C
    assert device_checksum(h, buf, n) == flipped
    h.close()


def test_checksum_captured_in_a_graph_replays_on_new_bytes():
    n = 70001
    stream = torch.cuda.Stream()
    h = _lib.Handle(0, stream.cuda_stream)
    rng = np.random.default_rng(8)
    buf = torch.zeros(n + GUARD, dtype=torch.uint8, device="cuda")
    out = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
        h.call("ivit_constants_checksum", P(buf), n, P(out))
    for _ in range(3):
        data = rng.integers(0, 256, n, dtype=np.uint8)
        buf[:n] = dev(data)
        out.fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert int(out.cpu().numpy().view(np.uint64)[0]) == mf.checksum_reference(data)
    h.close()


def test_checksum_verifies_an_uploaded_blob(tmp_root):
    g, cfg, eng, path, _ = model("micro_swin_b2", tmp_root)
    data = open(path, "rb").read()
    blob_offset, blob_bytes = struct.unpack_from("<QQ", data, 32)
    blob_sum = struct.unpack_from("<Q", data, 72)[0]
    host = np.frombuffer(data, np.uint8, blob_bytes, blob_offset).copy()
    h = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    there = torch.zeros(blob_bytes, dtype=torch.uint8, device="cuda")
    h.call("ivit_constants_upload", _P(host.ctypes.data), blob_bytes, P(there))
    assert device_checksum(h, there, blob_bytes) == blob_sum == mf.checksum_reference(host)
    there[12345] ^= 0x40
    assert device_checksum(h, there, blob_bytes) != blob_sum
    # the engine's own blob is the core part of the file's
    core = struct.unpack_from("<Q", data, 48)[0]
    assert device_checksum(h, eng.blob, eng.blob.numel()) == mf.checksum_reference(host[:core]) and eng.blob.numel() == core
    h.close()


# ---------------------------------------------------------------- the example: no Python in the process
def test_classify_example_prints_what_predict_returns(tmp_root, tmp_path):
    """examples/classify.c, built by build() next to the library, as a fresh child process on the deit_tiny file and its golden
    image written as raw int8.  A missing binary fails: the example is part of the feature."""
    g, cfg, eng, path, _ = model("deit_tiny_b1", tmp_root)
    exe = os.path.join(os.path.dirname(_lib.SO_PATH), "classify")
    assert os.path.exists(exe), "build() did not build examples/classify.c"
    images = iv.make_images_int8(cfg, int(g["batch"]), int(g["images_seed"]))
    images = np.concatenate([images, iv.make_images_int8(cfg, 2, seed=23)])
    B, k = images.shape[0], 5
    raw = tmp_path / "images.i8"
    raw.write_bytes(images.tobytes())
    run = subprocess.run([exe, path, str(raw), str(B), str(k)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stderr[-1000:])
    idx, val = eng.predict(dev(images), k=k, copy=True)
    lines = run.stdout.strip().split("\n")
    assert len(lines) == B
    for b, line in enumerate(lines):
        fields = line.split()
        assert int(fields[0]) == b and len(fields) == 1 + k
        got_idx = [int(f.split(":")[0]) for f in fields[1:]]
        got_val = np.array([f.split(":")[1] for f in fields[1:]], dtype=np.float32)
        assert got_idx == idx[b].cpu().tolist() and np.array_equal(got_val.view(np.uint32), val[b].cpu().numpy().view(np.uint32)), line
    assert np.array_equal(eng.last_logits[:int(g["batch"])].cpu().numpy(), g["logits_int"])


# ---------------------------------------------------------------- the tools
def _tool(name, monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))
    spec = importlib.util.spec_from_file_location("ivit_tools_" + name, os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_freeze_then_evaluate_with_a_model_file_prints_the_same_line(tmp_path, capsys, monkeypatch):
    g = load_golden("micro_vit2h_b3.npz")
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    golden = os.path.join(ROOT, "tests", "golden", "micro_vit2h_b3.npz")
    data, out = str(tmp_path / "data.npz"), str(tmp_path / "model.ivit")
    np.savez(data, images=iv.make_images_int8(cfg, 7, seed=31), labels=np.arange(7, dtype=np.int64) % cfg.num_classes)
    monkeypatch.setattr(sys, "argv", ["freeze.py", "--model", cfg.name, "--golden", golden, "--out", out])
    _tool("freeze", monkeypatch).main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["model"] == cfg.name and line["kind"] == "vit" and line["bytes"] == os.path.getsize(out)
    assert np.float32(line["input_scale"]) == g["scale/qact_input"]
    evaluate = _tool("evaluate", monkeypatch)
    lines = []
    for source in (["--model", cfg.name, "--golden", golden], ["--model-file", out]):
        monkeypatch.setattr(sys, "argv", ["evaluate.py", data] + source + ["--batch", "4", "--topk", "1", "3", "--loss"])
        evaluate.main()
        lines.append(capsys.readouterr().out)
    assert lines[0] == lines[1] and json.loads(lines[0].splitlines()[0])["n"] == 7
    monkeypatch.setattr(sys, "argv", ["evaluate.py", data, "--model", cfg.name, "--model-file", out])
    with pytest.raises(SystemExit):
        evaluate.main()
    sys.modules.pop("evaluate", None)
