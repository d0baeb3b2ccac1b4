"""Stand-alone timings behind the class-token tail of the last ViT block (csrc/ivit_model.h, cls_tail).
usage: python tools/cls_tail_bench.py [B] [H] [T]      default 256 6 197 (DeiT-S b256)
  1. the row-table attention (v row-major): whole-T launch, class-token launch with and without the identity-row copy, the copy as a
     launch of its own (ivit_gather_rows_i16), and the two launches back to back;
  2. at width 384 only: LayerNorm + fused Mlp at M = B rows as two launches against the LayerNorm-headed launch (which the library
     issues on the role-split kernel only: forced here with ivit_mlp_plan_select).
The candidates alternate (three rounds of 50 launches each, in turn); the medians are printed."""
import ctypes, sys, os
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ivit_amd as iv
from ivit_amd import _lib
_P = ctypes.c_void_p
B, Hh, T = [int(v) for v in sys.argv[1:4]] + [256, 6, 197][len(sys.argv) - 1:]
dh, D = 64, Hh * 64
Hd = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
rng = np.random.default_rng(0)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
P = lambda t: _P(t.data_ptr())
dyv = lambda d: _lib.Dyadic(float(d[0, 0]), float(d[0, 1]))


def timeit(f, n=50):
    for _ in range(3): f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): f()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1000


def medians(cands):
    return np.median([[timeit(f) for f in cands] for _ in range(3)], axis=0)


q = dev(rng.normal(0, 30, (B * Hh, T, dh)).clip(-127, 127).astype(np.int8))
k = dev(rng.normal(0, 30, (B * Hh, T, dh)).clip(-127, 127).astype(np.int8))
v = dev(rng.integers(-128, 128, (B * Hh, T, dh), dtype=np.int8))
x16 = dev(rng.integers(-30000, 30000, (B * T, D)).astype(np.int16))
s = np.float32(0.1947)
tabs = iv.freeze.shiftmax_tables(s)
rt = torch.empty(256, 64, dtype=torch.float32, device="cuda")
Hd.call("ivit_shiftmax_rowtable", P(dev(tabs["aq"])), P(dev(tabs["t"])), P(dev(tabs["cls"])), int(tabs["NC"]), int(tabs["t"].size), int(tabs["dmin"]), P(rt))
dqk = iv.freeze.dyadic(np.float32(6e-4), s); dpv = iv.freeze.dyadic(np.float32(3e-6), np.float32(9e-3))
full = torch.empty(B, T, D, dtype=torch.int8, device="cuda")
cc = torch.empty(B, D, dtype=torch.int8, device="cuda"); xc = torch.empty(B, D, dtype=torch.int16, device="cuda")
head = (P(q), P(k), P(v), dyv(dqk), float(s), P(rt), int(tabs["dmin"]), dyv(dpv))
whole = lambda: Hd.call("ivit_attention_fused_rowlut", *head, P(full), B, Hh, T, dh, 0)
cls_x = lambda: Hd.call("ivit_attention_fused_rowlut_cls", *head, P(cc), P(x16), P(xc), B, Hh, T, dh, 0)
cls_0 = lambda: Hd.call("ivit_attention_fused_rowlut_cls", *head, P(cc), None, None, B, Hh, T, dh, 0)
gather = lambda: Hd.call("ivit_gather_rows_i16", P(x16), B, D, T * D, P(xc))
both = lambda: (cls_0(), gather())
t = medians([whole, cls_x, cls_0, gather, both])
print(f"attention B {B} H {Hh} T {T}: whole {t[0]:.1f} us, class-token with the identity-row copy {t[1]:.1f} us, without {t[2]:.1f} us, "
      f"gather launch alone {t[3]:.1f} us, class-token + gather as two launches {t[4]:.1f} us", flush=True)

if D == 384:
    C, HD = 384, 1536
    w1 = dev(rng.integers(-128, 128, (HD, C), dtype=np.int8)); b1 = dev(rng.integers(-3000, 3000, HD).astype(np.int32))
    w2 = dev(rng.integers(-128, 128, (C, HD), dtype=np.int8)); b2 = dev(rng.integers(-3000, 3000, C).astype(np.int32))
    d1 = dev(iv.freeze.dyadic((10 ** rng.uniform(-5.6, -5.2, HD)).astype(np.float32), np.float32(0.012)))
    d2 = dev(iv.freeze.dyadic((10 ** rng.uniform(-5.9, -5.5, C)).astype(np.float32), np.float32(2e-4)))
    dm = iv.freeze.dyadic(np.float32(2e-4), np.float32(3.1e-4)); dr = iv.freeze.dyadic(np.float32(2.7e-4), np.float32(3.1e-4))
    tab = torch.empty(65536, dtype=torch.int8, device="cuda")
    Hd.call("ivit_shiftgelu_build_table", 0.03, dyv(iv.freeze.dyadic(np.float32(0.03 * 2.0 ** -7), np.float32(0.02))), P(tab))
    p1, p2, mp = _P(), _P(), _P()
    Hd.call("ivit_linear_plan_create", P(w1), P(b1), P(d1), HD, C, ctypes.byref(p1))
    Hd.call("ivit_linear_plan_create", P(w2), P(b2), P(d2), C, HD, ctypes.byref(p2))
    Hd.call("ivit_mlp_plan_create", p1, p2, ctypes.byref(mp))
    bias_int, sc = iv.freeze.layernorm_constants(rng.normal(1.0, 0.4, C).astype(np.float32), rng.normal(0.0, 0.5, C).astype(np.float32))
    bi_d, sc_d = dev(bias_int), dev(sc)
    dln = dev(iv.freeze.dyadic(sc, np.float32(0.031)))
    for M in sorted({128, B}):
        x = dev(rng.integers(-30000, 30000, (M, C)).astype(np.int16))
        a8 = torch.empty(M, C, dtype=torch.int8, device="cuda")
        o1 = torch.empty(M, C, dtype=torch.int16, device="cuda"); o2 = torch.empty_like(o1)

        def two():
            Hd.call("ivit_layernorm_requant", P(x), M, C, C, 2.5e-4, P(bi_d), P(sc_d), P(dln), P(a8))
            Hd.call("ivit_mlp_fused_planned", mp, P(a8), P(tab), dyv(dm), dyv(dr), P(x), P(o1), M)

        def headed():
            Hd.call("ivit_layernorm_mlp_fused_planned", mp, P(x), 2.5e-4, P(bi_d), P(sc_d), P(dln), P(a8), P(tab), dyv(dm), dyv(dr), P(o2), M)
        ln = lambda: Hd.call("ivit_layernorm_requant", P(x), M, C, C, 2.5e-4, P(bi_d), P(sc_d), P(dln), P(a8))
        assert Hd.lib.ivit_mlp_plan_select(mp, 0) == 0
        t2, tl = medians([two, ln])
        assert Hd.lib.ivit_mlp_plan_select(mp, 2) == 0       # role-split kernel whatever the size: the only one with the LayerNorm head
        (th,) = medians([headed])
        assert Hd.lib.ivit_mlp_plan_select(mp, 0) == 0
        print(f"width 384 M {M}: LayerNorm + fused Mlp, two launches {t2:.1f} us (LayerNorm alone {tl:.1f} us); LayerNorm-headed launch "
              f"(role-split kernel forced) {th:.1f} us; equal {bool(torch.equal(o1, o2))}", flush=True)
