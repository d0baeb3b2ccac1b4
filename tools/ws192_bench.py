"""Timings behind width 192 on the weights-in-registers GEMM (gemm_ws_qkv_kernel at K = 192, csrc/ivit_gemm_ws.h).
usage: python tools/ws192_bench.py [--parent-tree DIR] [--models deit_tiny:0,deit_tiny:256,deit_small:256] [--pairs 3] [--steps 100]
  1. stand-alone, one library: each new launch against the launches it replaces, which the same library still issues on a plan that
     was not prepared — norm1 + qkv (v row-major and v^T) against ivit_layernorm_requant + ivit_linear_i8_qkv_planned, the qkv layer
     alone, proj + residual, and Swin's plain 8-bit norm1 + qkv — at 197, 50 432 and 200 704 tokens.  The candidates alternate (three
     rounds of 50 launches each, in turn); medians and the min-max spread over the rounds are printed.
  2. with --parent-tree (a built checkout of the parent commit): whole models through each tree's own bench.py, one process per run,
     parent / new in turn; ms per step of every run, medians and ranges."""
import argparse, ctypes, json, os, subprocess, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def standalone():
    import torch
    import ivit_amd as iv
    from ivit_amd import _lib
    _P = ctypes.c_void_p
    Hd = _lib.Handle(0, torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    P = lambda t: _P(t.data_ptr())
    dyv = lambda d: _lib.Dyadic(float(d[0, 0]), float(d[0, 1]))
    K, Hh, dh, T = 192, 3, 64, 197

    def timeit(f, n=50):
        for _ in range(3): f()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n): f()
        b.record(); torch.cuda.synchronize()
        return a.elapsed_time(b) / n * 1000

    def report(title, cands):
        t = np.array([[timeit(f) for _, f in cands] for _ in range(3)])
        print(title + ": " + "; ".join(f"{n} {np.median(t[:, i]):.1f} us ({t[:, i].min():.1f}-{t[:, i].max():.1f})" for i, (n, _) in enumerate(cands)), flush=True)

    def lin(N):
        w = dev(np.rint(rng.normal(0, 45, (N, K)).clip(-128, 127)).astype(np.int8)); b = dev(rng.integers(-2 ** 14, 2 ** 14, N).astype(np.int32))
        return w, b

    bias_int, sc = iv.freeze.layernorm_constants(rng.normal(1.0, 0.4, K).astype(np.float32), rng.normal(0.0, 0.5, K).astype(np.float32))
    bi_d, sc_d, dln = dev(bias_int), dev(sc), dev(iv.freeze.dyadic(sc, np.float32(0.031)))
    wq, bq = lin(3 * K); dq = dev(iv.freeze.dyadic((10 ** rng.uniform(-5.5, -5, 3 * K)).astype(np.float32), np.float32(3e-3)))
    wp, bp = lin(K); dp = dev(iv.freeze.dyadic((10 ** rng.uniform(-5.5, -5, K)).astype(np.float32), np.float32(2e-4)))
    dm = iv.freeze.dyadic(np.float32(2e-4), np.float32(3.1e-4)); dr = iv.freeze.dyadic(np.float32(2.7e-4), np.float32(3.1e-4))
    q_plain, q_ws = Hd.linear_plan(P(wq), P(bq), P(dq), 3 * K, K), Hd.linear_plan(P(wq), P(bq), P(dq), 3 * K, K)
    p_plain, p_ws = Hd.linear_plan(P(wp), P(bp), P(dp), K, K), Hd.linear_plan(P(wp), P(bp), P(dp), K, K)
    Hd.call("ivit_linear_plan_prepare_ws", q_ws.p); Hd.call("ivit_linear_plan_prepare_ws", p_ws.p)
    for B in (1, 256, 1024):
        M, ld = B * T, (T + 15) // 16 * 16
        x16 = dev(rng.integers(-26000, 26000, (M, K)).astype(np.int16))
        a8 = torch.empty(M, K, dtype=torch.int8, device="cuda")
        q, k = (torch.empty(B * Hh * T, dh, dtype=torch.int8, device="cuda") for _ in range(2))
        v = torch.zeros(B * Hh * dh, ld, dtype=torch.int8, device="cuda")      # large enough for both layouts (ld >= T)
        ln = lambda: Hd.call("ivit_layernorm_requant", P(x16), M, K, K, 7.3e-4, P(bi_d), P(sc_d), P(dln), P(a8))
        for ldv in (0, ld):
            two = lambda: (ln(), Hd.call("ivit_linear_i8_qkv_planned", q_plain.p, P(a8), P(q), P(k), P(v), B, T, Hh, dh, ldv))
            old = lambda: Hd.call("ivit_linear_i8_qkv_planned", q_plain.p, P(a8), P(q), P(k), P(v), B, T, Hh, dh, ldv)
            new = lambda: Hd.call("ivit_linear_i8_qkv_planned", q_ws.p, P(a8), P(q), P(k), P(v), B, T, Hh, dh, ldv)
            one = lambda: Hd.call("ivit_layernorm_linear_i8_qkv_ldv_planned", q_ws.p, P(x16), 7.3e-4, P(bi_d), P(sc_d), P(dln), P(q), P(k), P(v), B, T, Hh, dh, ldv)
            report(f"M {M} ldv {ldv}", [("LayerNorm + qkv, two launches", two), ("one launch", one), ("LayerNorm alone", ln), ("qkv alone, plan as created", old),
                                        ("qkv alone, prepared", new)])
        if B == 1024:       # Swin-T b256 stage 1 (200 704 tokens; 201 728 here): the plain 8-bit layer
            o8 = torch.empty(M, 3 * K, dtype=torch.int8, device="cuda")
            two = lambda: (ln(), Hd.call("ivit_linear_i8_requant_planned", q_plain.p, P(a8), 8, P(o8), M))
            one = lambda: Hd.call("ivit_layernorm_linear_i8_requant_planned", q_ws.p, P(x16), 7.3e-4, P(bi_d), P(sc_d), P(dln), P(o8), M)
            report(f"M {M} plain 8-bit [M, 576]", [("LayerNorm + layer, two launches", two), ("one launch", one)])
        ctx = dev(rng.integers(-128, 128, (M, K), dtype=np.int8))
        o16 = torch.empty(M, K, dtype=torch.int16, device="cuda")
        old = lambda: Hd.call("ivit_linear_i8_requant_residual_planned", p_plain.p, P(ctx), dyv(dm), dyv(dr), P(x16), P(o16), M)
        new = lambda: Hd.call("ivit_linear_i8_requant_residual_planned", p_ws.p, P(ctx), dyv(dm), dyv(dr), P(x16), P(o16), M)
        report(f"M {M} proj + residual 192 -> 192", [("plan as created", old), ("prepared", new)])
    for p in (q_plain, q_ws, p_plain, p_ws):
        p.close()


def models(parent_tree, specs, pairs, steps):
    def run(tree, model, batch):
        cmd = [sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "10", "--model", model]
        if batch:
            cmd += ["--batch", str(batch)]
        out = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            raise SystemExit(f"bench.py failed ({out.returncode}): {out.stderr[-2000:]}")
        return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    for spec in specs:
        model, batch = spec.split(":")
        rows = []
        for i in range(pairs):
            a, b = run(parent_tree, model, int(batch)), run(ROOT, model, int(batch))
            rows.append((a["ms_per_step"], b["ms_per_step"]))
            print(f"{model} batch {batch or 'default'} pair {i + 1}: parent {a['ms_per_step']:.4f} ms, new {b['ms_per_step']:.4f} ms, "
                  f"gain {100 * (a['ms_per_step'] / b['ms_per_step'] - 1):.2f} %", flush=True)
        r = np.array(rows)
        print(f"{model} batch {batch or 'default'}: medians parent {np.median(r[:, 0]):.4f} new {np.median(r[:, 1]):.4f} ms; "
              f"parent {r[:, 0].min():.4f}-{r[:, 0].max():.4f}, new {r[:, 1].min():.4f}-{r[:, 1].max():.4f}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--models", default="deit_tiny:0,deit_tiny:256,deit_small:256")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--no-standalone", action="store_true")
    args = ap.parse_args()
    if not args.no_standalone:
        standalone()
    if args.parent_tree:
        models(os.path.abspath(args.parent_tree), args.models.split(","), args.pairs, args.steps)
