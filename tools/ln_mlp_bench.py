"""Stand-alone timings of norm2 + Mlp as ONE launch of the lock-step kernel (ivit_layernorm_mlp_lockstep_planned) against the two
launches it replaces (ivit_layernorm_requant, then ivit_mlp_fused_planned on the lock-step kernel).
usage: python tools/ln_mlp_bench.py [width:M ...]      default 192:197 192:50432 192:200704 384:256 384:788 384:20480
The candidates alternate (three rounds of 50 launches each, in turn); the medians are printed, one line per shape, and the outputs of
the two forms are compared."""
import ctypes, sys, os
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ivit_amd as iv
from ivit_amd import _lib
_P = ctypes.c_void_p
shapes = [tuple(int(v) for v in a.split(":")) for a in sys.argv[1:]] or [(192, 197), (192, 50432), (192, 200704), (384, 256), (384, 788), (384, 20480)]
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


plans = {}
for C in sorted({c for c, _ in shapes}):
    HD = 4 * C
    w1 = dev(rng.integers(-128, 128, (HD, C), dtype=np.int8)); b1 = dev(rng.integers(-3000, 3000, HD).astype(np.int32))
    w2 = dev(rng.integers(-128, 128, (C, HD), dtype=np.int8)); b2 = dev(rng.integers(-3000, 3000, C).astype(np.int32))
    d1 = dev(iv.freeze.dyadic((10 ** rng.uniform(-5.6, -5.2, HD)).astype(np.float32), np.float32(0.012)))
    d2 = dev(iv.freeze.dyadic((10 ** rng.uniform(-5.9, -5.5, C)).astype(np.float32), np.float32(2e-4)))
    p1, p2, mp = _P(), _P(), _P()
    Hd.call("ivit_linear_plan_create", P(w1), P(b1), P(d1), HD, C, ctypes.byref(p1))
    Hd.call("ivit_linear_plan_create", P(w2), P(b2), P(d2), C, HD, ctypes.byref(p2))
    Hd.call("ivit_mlp_plan_create", p1, p2, ctypes.byref(mp))
    assert Hd.lib.ivit_mlp_plan_select(mp, 1) == 0          # both forms on the lock-step kernel
    bias_int, sc = iv.freeze.layernorm_constants(rng.normal(1.0, 0.4, C).astype(np.float32), rng.normal(0.0, 0.5, C).astype(np.float32))
    plans[C] = (mp, dev(bias_int), dev(sc), dev(iv.freeze.dyadic(sc, np.float32(0.031))), (w1, b1, w2, b2, d1, d2))
dm = iv.freeze.dyadic(np.float32(2e-4), np.float32(3.1e-4)); dr = iv.freeze.dyadic(np.float32(2.7e-4), np.float32(3.1e-4))
tab = torch.empty(65536, dtype=torch.int8, device="cuda")
Hd.call("ivit_shiftgelu_build_table", 0.03, dyv(iv.freeze.dyadic(np.float32(0.03 * 2.0 ** -7), np.float32(0.02))), P(tab))

for C, M in shapes:
    mp, bi_d, sc_d, dln, _ = plans[C]
    x = dev(rng.integers(-30000, 30000, (M, C)).astype(np.int16))
    a8 = torch.empty(M, C, dtype=torch.int8, device="cuda")
    o1 = torch.empty(M, C, dtype=torch.int16, device="cuda"); o2 = torch.empty_like(o1)
    ln = lambda: Hd.call("ivit_layernorm_requant", P(x), M, C, C, 2.5e-4, P(bi_d), P(sc_d), P(dln), P(a8))
    mlp = lambda: Hd.call("ivit_mlp_fused_planned", mp, P(a8), P(tab), dyv(dm), dyv(dr), P(x), P(o1), M)
    two = lambda: (ln(), mlp())
    one = lambda: Hd.call("ivit_layernorm_mlp_lockstep_planned", mp, P(x), 2.5e-4, P(bi_d), P(sc_d), P(dln), P(tab), dyv(dm), dyv(dr), P(o2), M)
    t2, t1, tl, tm = medians([two, one, ln, mlp])
    print(f"width {C} M {M}: LayerNorm + fused Mlp, two launches {t2:.1f} us (LayerNorm alone {tl:.1f}, Mlp alone {tm:.1f}); one launch "
          f"{t1:.1f} us ({(t1 / t2 - 1) * 100:+.1f} %); equal {bool(torch.equal(o1, o2))}", flush=True)
