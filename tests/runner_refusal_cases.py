"""The refused calls of the runner entries, stated once for tools/make_runner_refusals_fixture.py (which records what a library
answers) and tests/test_runner_refusals_gpu.py (which holds a library to the record).

An entry is a list of parameters in the order of its prototype; `refusals(spec)` gives, per entry, calls that each break exactly ONE
rule: a pointer null, `bytes` one short, the workspace misaligned, a bad slice count, two of the entry's arrays laid over one
another, a bad index list, a bad mode / layout / k, hid32 misaligned, val given in IVIT_CLASSMAP_GIVEN mode.  A pointer the entry
takes as optional is not nulled (that call is legal and launches).

Every device array of an entry lies at the start of an arena of its own, 2 * `big` bytes filled with 0x5A, where `big` is more than
the largest extent among the entry's arrays: a substituted pointer (the second array of a pair put on the first one's start, or on
its last bytes) then lies inside an arena with room for the substituted extent, so a call that is wrongly NOT refused still
touches only memory the caller of this module owns."""
import ctypes

import numpy as np
import torch

import ivit_amd as iv
from ivit_amd import _lib

FILL = 0x5A
B, K = 2, 3
MODELS = ("micro_vit_b2.npz", "micro_swin_b2.npz")


class Arr:
    """a device array of `nbytes`: `table` — it is in the entry's overlap table; `optional` — null is legal; `read_only` — the
    entry only reads it; `init` — a tensor whose bytes it holds (else the fill); `absent` — the unmodified call passes null"""

    def __init__(self, nbytes, table=True, optional=False, read_only=False, init=None, absent=False):
        self.nbytes, self.table, self.optional, self.read_only, self.init, self.absent = int(nbytes), table, optional, read_only, init, absent


class Ptr:
    """a device pointer into the engine's own constants, or a host pointer: nulled in its turn (unless null is legal), never moved"""

    def __init__(self, value, optional=False):
        self.value, self.optional = value, optional


class Host:
    """a host index list; the parameter behind it is its length"""

    def __init__(self, sites, total):
        self.sites, self.total = tuple(sites), total


def engine(fname, golden, scales):
    g = golden(fname)
    if str(g["cfg_name"]) in iv.SWIN_CONFIGS:
        from ivit_amd.swin_engine import SwinEngine
        cfg = iv.SWIN_CONFIGS[str(g["cfg_name"])]
        eng = SwinEngine(cfg, iv.make_swin_weights(cfg, int(g["seed"])), scales(g))
    else:
        from ivit_amd.engine import ViTEngine
        cfg = iv.CONFIGS[str(g["cfg_name"])]
        eng = ViTEngine.from_float(cfg, iv.make_vit_weights(cfg, int(g["seed"])), scales(g))
    assert int(g["batch"]) == B
    imgs = torch.from_numpy(iv.make_images_int8(cfg, B, int(g["images_seed"]))).cuda()
    return g, cfg, eng, imgs


def entries(cfg, eng, imgs):
    """{key: (C symbol, [(parameter, value)])} for every eager runner entry of the model at batch B, one slice"""
    swin = eng.PREFIX == "ivit_swin"
    need = ctypes.c_size_t()
    eng._entry("_workspace_bytes", eng.model, B, 1, ctypes.byref(need))
    need, ncls = need.value, cfg.num_classes
    assert ncls >= K
    head_scale = Ptr(eng.ptr("head.scale").value)
    labels = torch.arange(B, dtype=torch.int64, device="cuda") % ncls

    def fwd(logits_optional=False):
        return [("m", Ptr(eng.model.value)), ("images", Arr(imgs.numel(), read_only=True, init=imgs)), ("batch", B), ("nslices", 1),
                ("workspace", Arr(need)), ("bytes", need), ("logits", Arr(4 * B * ncls, optional=logits_optional))]
    out = {"workspace_bytes": (eng.PREFIX + "_workspace_bytes", [("m", Ptr(eng.model.value)), ("batch", B), ("nslices", 1), ("bytes_out", Ptr(None))]),
           "forward": (eng.PREFIX + "_forward", fwd()),
           "predict": (eng.PREFIX + "_predict", fwd() + [("head_scale", head_scale), ("k", K), ("idx", Arr(4 * B * K)),
                                                         ("val", Arr(4 * B * K, optional=True))]),
           "score": (eng.PREFIX + "_score", fwd() + [("head_scale", head_scale), ("labels", Ptr(labels)),
                                                     ("rank", Arr(4 * B, table=False, optional=True)), ("nll", Arr(8 * B, table=False, optional=True))]),
           "features": (eng.PREFIX + "_features", fwd(True) + [("feat8", Arr(B * eng.num_features, table=False)), ("scale", float(eng.feature_scale_host())),
                                                               ("mode", _lib.IVIT_FEATURES_DEQUANT), ("feat32", Arr(4 * B * eng.num_features, table=False, optional=True))])}
    sites = eng._hidden_sites()
    planes = [eng._hidden_plane(i) for i in range(sites)]
    n16 = sum(B * T * C for T, C, _ in planes)
    out["hidden_states"] = (eng.PREFIX + "_hidden_states", fwd(True) + [
        ("stages_host" if swin else "blocks_host", Host(range(sites), sites)), ("n", sites), ("hid16", Arr(2 * n16)), ("layout", _lib.IVIT_HIDDEN_TOKENS),
        ("hid32", Arr(4 * n16, optional=True))])
    if swin:
        g = cfg.grid >> (cfg.num_layers - 1)
        L, C = g * g, eng.num_features
        classes = torch.tensor([[0, 1, 2], [2, 1, 0]], dtype=torch.int32, device="cuda")
        for key, mode, given in (("class_map_topk", _lib.IVIT_CLASSMAP_TOPK, False), ("class_map_given", _lib.IVIT_CLASSMAP_GIVEN, True)):
            out[key] = ("ivit_swin_class_map", fwd(given) + [
                ("head_scale", Ptr(head_scale.value, optional=given)), ("mode", mode), ("k", K),
                ("idx", Arr(4 * B * K, read_only=given, init=classes if given else None)), ("val", Arr(4 * B * K, optional=True, absent=given)),
                ("tok8", Arr(B * L * C)), ("class_scale", Ptr(eng.class_scale)), ("cam32", Arr(4 * B * K * L)), ("map32", Arr(4 * B * K * L))])
    else:
        H, T = cfg.num_heads, cfg.num_tokens
        for key, mode, per in (("attention_heads", _lib.IVIT_ATTNMAP_HEADS, H), ("attention_mean", _lib.IVIT_ATTNMAP_MEAN, 1)):
            out[key] = ("ivit_vit_attention", fwd(True) + [
                ("blocks_host", Host(range(cfg.depth), cfg.depth)), ("n", cfg.depth), ("attn16", Arr(2 * cfg.depth * B * H * T)), ("mode", mode),
                ("map32", Arr(4 * cfg.depth * B * per * (T - 1), optional=True))])
    return out


def arenas(params):
    """{parameter: uint8 tensor} for every device array of the entry, and `big`"""
    arrs = {n: v for n, v in params if isinstance(v, Arr)}
    big = (max([a.nbytes for a in arrs.values()] + [0]) + 4096 + 255) // 256 * 256
    mem = {}
    for n, a in arrs.items():
        mem[n] = torch.full((2 * big,), FILL, dtype=torch.uint8, device="cuda")
        assert mem[n].data_ptr() % 256 == 0
        if a.init is not None:
            mem[n][:a.nbytes].copy_(a.init.reshape(-1).view(torch.uint8))
    return mem, big


def refusals(params, max_slices):
    """[(case name, {parameter: replacement})]: None — null; ("at", arena, offset) — a pointer into that arena; else the value"""
    p = dict(params)
    arrs = [(n, v) for n, v in params if isinstance(v, Arr)]
    cases = [("m null", {"m": None})]
    for n, v in params[1:]:
        if isinstance(v, Host) or (isinstance(v, Ptr) and not v.optional) or (isinstance(v, Arr) and not v.optional and not v.absent):
            cases.append((f"{n} null", {n: None}))
    if "bytes" in p:
        cases += [("bytes one short", {"bytes": p["bytes"] - 1}), ("workspace misaligned by 16", {"workspace": ("at", "workspace", 16)})]
    else:
        cases.append(("batch 0", {"batch": 0}))
    cases += [(f"nslices {ns}", {"nslices": ns}) for ns in (0, B + 1, max_slices + 1)]
    table = [(n, v) for n, v in arrs if v.table and not v.absent]
    for i, (a, va) in enumerate(table):
        for b, vb in table[i + 1:]:
            if va.read_only and vb.read_only:
                continue
            for at in sorted({0, max(0, va.nbytes - 16) // 256 * 256}):
                cases.append((f"{b} over {a} at {at}", {b: ("at", a, at)}))
    for n, v in params:
        if isinstance(v, Host):
            t = v.total
            assert t == 2 and v.sites == (0, 1)
            cases += [(f"{n} empty", {n: (0,), "n": 0}), (f"{n} too long", {n: (0, 1, 2), "n": 3}), (f"{n} descending", {n: (1, 0)}),
                      (f"{n} repeated", {n: (0, 0)}), (f"{n} out of range", {n: (0, t)}), (f"{n} negative", {n: (-1, 1)})]
    for n in ("mode", "layout"):
        if n in p:
            cases += [(f"{n} 7", {n: 7}), (f"{n} -1", {n: -1})]
    if "k" in p:
        cases += [("k 0", {"k": 0}), ("k 17", {"k": 17})]
    if "hid32" in p:
        cases.append(("hid32 misaligned by 4", {"hid32": ("at", "hid32", 4)}))
    if "rank" in p:
        cases.append(("rank and nll null", {"rank": None, "nll": None}))
    if "val" in p and p["val"].absent:
        cases.append(("val given in GIVEN mode", {"val": ("at", "val", 0)}))
    return cases


def call_args(params, mem, change=None):
    """the ctypes arguments of one call, and what must stay alive while it runs"""
    change, args, keep = change or {}, [], []
    for n, v in params:
        r = change.get(n, v)
        if r is None:
            args.append(None)
        elif isinstance(r, Arr):
            args.append(None if r.absent else ctypes.c_void_p(mem[n].data_ptr()))
        elif isinstance(r, Ptr):
            if n == "bytes_out":
                keep.append(ctypes.c_size_t())
                args.append(ctypes.byref(keep[-1]))
            else:
                keep.append(r.value)
                args.append(ctypes.c_void_p(r.value.data_ptr()) if isinstance(r.value, torch.Tensor) else ctypes.c_void_p(r.value))
        elif isinstance(r, Host) or (isinstance(r, tuple) and r[:1] != ("at",)):
            idx = r.sites if isinstance(r, Host) else r
            keep.append((ctypes.c_int * max(len(idx), 1))(*idx))
            args.append(keep[-1])
        elif isinstance(r, tuple):
            args.append(ctypes.c_void_p(mem[r[1]].data_ptr() + r[2]))
        else:
            args.append(r)
    return args, keep


def run(eng, symbol, params, mem, change=None):
    """(status, ivit_last_error) of one call on the current stream"""
    args, keep = call_args(params, mem, change)
    eng._use_current_stream()
    st = getattr(eng.h.lib, symbol)(*args)
    del keep
    return int(st), eng.h.lib.ivit_last_error(eng.h.h).decode()


def good_logits(params, mem, ncls):
    """the logits of the unmodified call, or None where the entry has none"""
    if "logits" not in dict(params):
        return None
    return mem["logits"][:4 * B * ncls].view(torch.int32).view(B, ncls).cpu().numpy().astype(np.int64)
