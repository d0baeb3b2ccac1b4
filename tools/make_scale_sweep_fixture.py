"""Generate tests/golden/scale_sweep.npz: the reference's own operators swept over activation scales and requant
multipliers (tests/test_scale_sweep_cpu.py, tests/test_scale_sweep_gpu.py).

Runs ONLY in the build container (needs the reference tree + torch CPU), like tools/make_golden.py.  The fixture is data:
the input blocks of tests/scale_sweep.py (each stored once), the scale lists, per scale an order-sensitive checksum of
the integers the reference produced, and the full outputs at eight scales per operator so that a failure can be
localised.  The file is written with fixed zip timestamps, so a rerun is byte-identical.

    python tools/make_scale_sweep_fixture.py
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, _HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ivit_amd as iv  # noqa: E402
import ref_harness as rh  # noqa: E402
import scale_sweep as sw  # noqa: E402
from make_golden import frozen_act  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "scale_sweep.npz")
f32 = np.float32


def neighbours(v):
    v = f32(v)
    return [np.nextafter(v, f32(0)), np.nextafter(v, f32(np.inf))]


def elementwise_scales():
    rng = np.random.Generator(np.random.PCG64(4321))
    s = [f32(2.0 ** -k) for k in range(10)]
    s += [f32(f32(1) / f32(k)) for k in (3, 5, 7, 10, 100, 127, 128, 255)]
    for v in (1 / 2, 1 / 4, 1 / 8, 1 / 16, 1 / 64):       # floor(-1/s) flips between the two neighbours
        s += neighbours(v)
    s += [f32(3.0), f32(4.7), f32(8.0)]
    s += list((10 ** rng.uniform(-3.2, 0.4, 150 - len(s))).astype(f32))
    return np.asarray(s, f32)


def ln_scales():
    rng = np.random.Generator(np.random.PCG64(4322))
    return (10 ** rng.uniform(-6, np.log10(3e-3), 48)).astype(f32)


def attention_scales():
    """60 log-uniform scales in [0.02, 0.6], then the row-table boundary and one scale without tables.  A line of the
    Shiftmax row table has R = 1 - dmin entries, and dmin is decided by x0 = floor(-1/s): R is 43, 54, 64, 74, 85 for
    x0 = -4 .. -8 — 65 is not attainable.  The boundary of ivit_shiftmax_rowtable (R <= 64) is therefore the flip of x0
    from -6 to -7 at s = 1/6: the two adjacent float32 values on either side of it are taken, the smallest scale with
    R = 64 and the largest with R = 74.  Last comes a scale whose two-level tables do not fit their budget."""
    rng = np.random.Generator(np.random.PCG64(4323))
    s = list((10 ** rng.uniform(np.log10(0.02), np.log10(0.6), 60)).astype(f32))
    c = f32(1.0 / 6.0)
    for _ in range(4):
        c = np.nextafter(c, f32(0))
    r64 = rnext = None
    for _ in range(9):                                     # ascending through 1/6
        t = iv.freeze.shiftmax_tables(c)
        assert t is not None
        if t["R"] > 64:
            rnext = c
        elif r64 is None:
            assert t["R"] == 64
            r64 = c
        c = np.nextafter(c, f32(1))
    assert r64 is not None and rnext is not None and r64 == np.nextafter(rnext, f32(1))
    none = next(v for v in sorted(s) if iv.freeze.shiftmax_tables(v) is None)
    none = np.nextafter(f32(none), f32(0))                 # a value of its own, not a second copy of a list member
    assert iv.freeze.shiftmax_tables(none) is None
    return np.asarray(s + [r64, rnext, none], f32)


def full_idx(n):
    """the eight scales (smallest, largest and six between, by value order position) whose outputs are kept whole"""
    return np.unique(np.linspace(0, n - 1, 8).round().astype(np.int64))


def sub(keep, k):
    """k of the kept scales, the extremes first (the wide outputs are kept at fewer scales: the file stays below 1 MiB)"""
    pos = {1: [0], 2: [0, -1], 3: [0, len(keep) // 2, -1], 4: [0, 2, 5, -1]}.get(k)
    return keep if pos is None else keep[pos]


def run_shiftmax(models, x, s, bits, mask=None):
    mod = models.IntSoftmax(bits)
    xt = torch.from_numpy(x.astype(np.float32)) * torch.tensor(s)
    if mask is not None:      # swin_quant.py:151-156: [B_/nW, nW, H, N, N] + mask[None, :, None]
        n = x.shape[-1]
        xt = (xt.view(-1, sw.MASK_NW, sw.MASK_H, n, n) + torch.from_numpy(mask).unsqueeze(1).unsqueeze(0)).view(-1, n)
    with torch.no_grad():
        y, so = mod(xt, torch.tensor(s))
    out = torch.round(y / so).numpy().astype(np.int64)
    assert out.min() >= 0 and out.max() <= 65535
    return out.astype(np.uint16)


def build(models):
    d = {}
    ew = elementwise_scales()
    at = attention_scales()
    lns = ln_scales()
    d["ew/scales"], d["attn/scales"], d["ln/scales"] = ew, at, lns
    order = np.argsort(ew, kind="stable")
    keep = order[full_idx(len(ew))]
    d["ew/full"] = keep.astype(np.int32)
    # ---- Shiftmax: every length at every elementwise scale; the 16-bit lengths at the attention scales too
    for n in sw.SHIFTMAX_N:
        x = sw.shiftmax_rows(n)
        bits = sw.SHIFTMAX_BITS[n]
        d[f"shiftmax/{n}/x"] = x
        cs = []
        for i, s in enumerate(ew):
            out = run_shiftmax(models, x, s, bits)
            cs.append(sw.csum(out))
            if i in sub(keep, {197: 2, 260: 1}.get(n, 8)):
                d[f"shiftmax/{n}/out/{i}"] = out.astype(np.uint8) if out.max() < 256 else out
        d[f"shiftmax/{n}/csum"] = np.asarray(cs, np.uint64)
        if bits == 16:
            d[f"shiftmax/{n}/attn_csum"] = np.asarray([sw.csum(run_shiftmax(models, x, s, 16)) for s in at], np.uint64)
    # ---- masked Shiftmax (Swin): x*s + mask
    x, mask = sw.masked_rows()
    d["masked/x"], d["masked/mask"] = x, mask
    cs = []
    for i, s in enumerate(ew):
        out = run_shiftmax(models, x, s, 8, mask)
        cs.append(sw.csum(out))
        if i in keep:
            d[f"masked/out/{i}"] = out.astype(np.uint8) if out.max() < 256 else out
    d["masked/csum"] = np.asarray(cs, np.uint64)
    # ---- ShiftGELU: the 32-bit product, its extremes, and QuantAct(8) at two output scales
    x = sw.gelu_block()
    d["gelu/x"] = x
    cs, lo, hi, so8, cs8 = [], [], [], [], []
    for i, s in enumerate(ew):
        mod = models.IntGELU()
        with torch.no_grad():
            y, so = mod(torch.from_numpy(x.astype(np.float32)) * torch.tensor(s), torch.tensor(s))
            prod = torch.round(y / so).numpy().astype(np.int64)
            row_so, row_cs = [], []
            for j, rel in enumerate((1.0, 0.37)):
                act = frozen_act(models, 8, f32(f32(s) * f32(rel)))
                y8, s8 = act(y, so)
                o8 = torch.round(y8 / s8).numpy().astype(np.int8)
                row_so.append(f32(s8.item()))
                row_cs.append(sw.csum(o8))
                if i in keep:
                    d[f"gelu/out8/{j}/{i}"] = o8
        assert np.abs(prod).max() < 2 ** 31
        cs.append(sw.csum(prod))
        lo.append(prod.min())
        hi.append(prod.max())
        so8.append(row_so)
        cs8.append(row_cs)
        if i in sub(keep, 3):
            d[f"gelu/prod/{i}"] = prod.astype(np.int32)
    d["gelu/csum"] = np.asarray(cs, np.uint64)
    d["gelu/min"], d["gelu/max"] = np.asarray(lo, np.int32), np.asarray(hi, np.int32)
    d["gelu/maxabs"] = np.maximum(-d["gelu/min"].astype(np.int64), d["gelu/max"].astype(np.int64)).astype(np.int32)
    d["gelu/s_out8"] = np.asarray(so8, f32)
    d["gelu/csum8"] = np.asarray(cs8, np.uint64)
    # ---- I-LayerNorm + per-channel QuantAct(8)
    lkeep = np.argsort(lns, kind="stable")[full_idx(len(lns))]
    d["ln/full"] = lkeep.astype(np.int32)
    for C in sw.LN_C:
        x, w, b = sw.ln_block(C)
        d[f"ln/{C}/x"], d[f"ln/{C}/w"], d[f"ln/{C}/b"] = x, w, b
        ln = models.IntLayerNorm(C)
        ln.weight.data = torch.from_numpy(w)
        ln.bias.data = torch.from_numpy(b)
        act = frozen_act(models, 8, f32(0.04))
        csz, cs8 = [], []
        for i, s in enumerate(lns):
            with torch.no_grad():
                y, sc = ln(torch.from_numpy(x[None].astype(np.float32)) * torch.tensor(s), torch.tensor(s))
                z = torch.round(y / sc.reshape(1, 1, -1)).numpy().astype(np.float64)[0]
                y8, so = act(y, sc)
                o8 = torch.round(y8 / so).numpy().astype(np.int8)[0]
            csz.append(sw.csum(z))
            cs8.append(sw.csum(o8))
            if i in sub(lkeep, 2 if C <= 96 else 1):
                d[f"ln/{C}/z/{i}"] = z.astype(np.float32)
            if i in sub(lkeep, 4 if C <= 128 else 2):
                d[f"ln/{C}/out8/{i}"] = o8
        d[f"ln/{C}/csum_z"] = np.asarray(csz, np.uint64)
        d[f"ln/{C}/csum8"] = np.asarray(cs8, np.uint64)
        d["ln/s_out"] = f32(so.item())
    # ---- the same on a TOKEN-contiguous input (Swin stage 0: flatten(2).transpose(1, 2)), two images of 49 tokens
    for C in sw.LN_TOKEN_C:
        x, w, b = sw.ln_token_block(C)
        ln = models.IntLayerNorm(C)
        ln.weight.data = torch.from_numpy(w)
        ln.bias.data = torch.from_numpy(b)
        act = frozen_act(models, 8, f32(0.04))
        xt = torch.from_numpy(np.ascontiguousarray(x.reshape(2, sw.LN_TOKENS, C).transpose(0, 2, 1)).astype(np.float32))
        xt = xt.transpose(1, 2)                              # [2, 49, C] with the token dimension contiguous
        csz, cs8 = [], []
        for i, s in enumerate(lns):
            with torch.no_grad():
                xs = xt * torch.tensor(s)
                assert xs.stride() == xt.stride() and xs.stride(1) == 1
                y, sc = ln(xs, torch.tensor(s))
                z = torch.round(y / sc.reshape(1, 1, -1)).numpy().astype(np.float64).reshape(-1, C)
                y8, so = act(y, sc)
                o8 = torch.round(y8 / so).numpy().astype(np.int8).reshape(-1, C)
            csz.append(sw.csum(z))
            cs8.append(sw.csum(o8))
            if i in sub(lkeep, 1):
                d[f"lntok/{C}/z/{i}"] = z.astype(np.float32)
        d[f"lntok/{C}/csum_z"] = np.asarray(csz, np.uint64)
        d[f"lntok/{C}/csum8"] = np.asarray(cs8, np.uint64)
    # ---- input QuantAct: the scale the module derives from its frozen range is the one recorded
    grid = sw.qin_grid()
    d["qin/grid"] = grid
    qs, cs = [], []
    for i, s in enumerate(ew):
        act = frozen_act(models, 8, s)
        with torch.no_grad():
            y, so = act(torch.zeros(1, 1))
            so = f32(so.item())
            y, so2 = act(torch.from_numpy(sw.qin_values(so))[None])
        assert f32(so2.item()) == so
        out = torch.round(y / so2).numpy().astype(np.int8)[0]
        qs.append(so)
        cs.append(sw.csum(out))
        if i in keep:
            d[f"qin/out/{i}"] = out
    d["qin/scales"] = np.asarray(qs, f32)
    d["qin/csum"] = np.asarray(cs, np.uint64)
    # ---- QuantAct requant: a multiplier sweep (per-channel s_pre = ratio * s_out, s_out = 2^-4)
    zi = sw.rq_identity()
    d["rq/z_id"] = zi
    for zname, zmax in sw.RQ_ZMAX.items():
        ratios = sw.rq_ratios(zmax)
        d[f"rq/{zname}/ratios"] = ratios
        d[f"rq/{zname}/z"] = sw.rq_block(zmax, ratios)
    for ci, (zname, bits, ident) in enumerate(sw.RQ_CASES):
        z = d[f"rq/{zname}/z"]
        s_pre = (d[f"rq/{zname}/ratios"] * sw.RQ_S_OUT).astype(f32)
        act = frozen_act(models, bits, sw.RQ_S_OUT)
        sp = torch.from_numpy(s_pre)
        xt = torch.from_numpy(z.astype(np.float64)).float() * sp.reshape(1, -1)
        assert np.array_equal(torch.round(xt / sp.reshape(1, -1)).numpy(), z.astype(np.float32))   # the reference sees z itself
        kw = {}
        if ident:
            s_id = np.array([sw.RQ_ID_RATIO[ident] * sw.RQ_S_OUT], f32)
            xi = torch.from_numpy(zi.astype(np.float32)) * torch.tensor(s_id[0])
            assert np.array_equal(torch.round(xi / torch.tensor(s_id[0])).numpy(), zi.astype(np.float32))
            kw = dict(identity=xi, identity_scaling_factor=torch.from_numpy(s_id))
        with torch.no_grad():
            y, so = act(xt, sp, **kw)
        assert f32(so.item()) == sw.RQ_S_OUT
        d[f"rq/out/{ci}"] = torch.round(y / so).numpy().astype(np.int8 if bits == 8 else np.int16)
    return d


def save_deterministic(path, d):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(d):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(d[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    models = rh.load_reference()
    torch.manual_seed(0)
    d = build(models)
    save_deterministic(OUT, d)
    print("scale_sweep.npz bytes", os.path.getsize(OUT), "arrays", len(d))


if __name__ == "__main__":
    main()
