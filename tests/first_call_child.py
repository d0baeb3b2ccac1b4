"""A process whose FIRST launch of a kernel is made inside a hipGraph capture (tests/test_stream_graph_contract_gpu.py::
test_first_call_of_a_process_inside_a_capture starts it as a fresh child).  launch_dyn (csrc/ivit_hip.hip) calls hipFuncSetAttribute
the first time a kernel asks for more than 64 KB of dynamic LDS on a device, and the runtime loads a kernel's code on its first
launch: both happen here between hipStreamBeginCapture and hipStreamEndCapture.  Three entries whose launch is above 64 KB:
    ivit_layernorm                      8 rows of C = 2056: 65 792 B (abi_cases.ln_lds_case); the replay must equal the ORACLE
    ivit_attention_fused_rowlut         T = 65: every launch of the row-table form is above 64 KB
    ivit_layernorm_mlp_fused_planned    a 384 -> 1536 -> 384 plan at M = 64
Each goes through abi_cases.check_stream_contract with eager_first=False: captured on a side stream (nothing runs before the graph is
launched), replayed, compared with an eager call made AFTER the replay, replayed on other inputs.  The handle lives on a stream of its
own, never on the default stream.  One JSON line per entry on stdout, {"entry": ..., "ok": true} or {"entry": ..., "error": message};
exit status 0 only if all three are ok.  The process stops at the first failure: nothing more is started on a device after one."""
import json
import sys
import time

import numpy as np

import abi_cases as A


def cases(H, rng, first):
    """-> [(entry, args, setup)]; first: the table the capture is made on (the LayerNorm rows are the oracle's case), otherwise the
    same calls with other contents drawn from rng"""
    import ivit_amd as iv
    I, O = A._io()
    R = lambda key: ("ref", key)                                                  # noqa: E731
    i8 = lambda *shape: rng.integers(-128, 128, shape, dtype=np.int8)             # noqa: E731
    cs = []
    x, bias_int, sc, _ = A.ln_lds_case(2056)
    if not first:
        x = rng.integers(-26000, 26000, x.shape).astype(np.int16)
    cs.append(("layernorm", [I(x), 8, 2056, A.LN_LDS_SCALE, I(bias_int), I(sc), O(np.zeros((8, 2056), np.float32))], None))
    tabs = iv.freeze.shiftmax_tables(A.ATT_SCALE)
    rowtab = iv.freeze.shiftmax_rowtable(tabs)
    B, Hh, T, dh, ld = 2, 2, 65, 64, 80
    vt = np.zeros((B * Hh, dh, ld), np.int8)
    vt[:, :, :T] = i8(B * Hh, dh, T)
    dqk, dpv = iv.freeze.dyadic(np.float32(2.2e-4), A.ATT_SCALE), iv.freeze.dyadic(np.float32(2.0 ** -15 * 0.1), np.float32(0.05))
    cs.append(("attention_fused_rowlut", [I(i8(B * Hh, T, dh)), I(i8(B * Hh, T, dh)), I(vt, T), A.dyv(dqk), float(A.ATT_SCALE), R("rt"), int(tabs["dmin"]),
                                          A.dyv(dpv), O(np.zeros((B, T, Hh * dh), np.int8)), B, Hh, T, dh, ld], A._setup(H, const=(("rt", rowtab),))))
    C, M = 384, 64
    lay = [("fc1", A._layer(rng, 4 * C, C, 8)), ("fc2", A._layer(rng, C, 4 * C, 16))]
    bi, scl, dln = A._ln(rng, C)
    dm, dr = iv.freeze.dyadic(np.float32(2e-4), np.float32(3.1e-4)), iv.freeze.dyadic(np.float32(2.7e-4), np.float32(3.1e-4))
    cs.append(("layernorm_mlp_fused_planned", [R("mlp"), I(A._x16(rng, M, C)), 2.5e-4, R("bi"), R("sc"), R("dln"), O(np.zeros((M, C), np.int8)), R("tab"),
                                               A.dyv(dm), A.dyv(dr), O(np.zeros((M, C), np.int16)), M],
               A._setup(H, lay, mlp=("fc1", "fc2"), select=2, gelu=True, const=(("bi", bi), ("sc", scl), ("dln", dln)))))
    return cs


def main():
    import torch
    from ivit_amd import _lib
    own = torch.cuda.Stream()
    ok = True
    with torch.cuda.stream(own):
        H = _lib.Handle(0, own.cuda_stream)
        mem = A.TorchMem()
        second = cases(H, np.random.default_rng(A.SECOND_SEED), False)
        for (name, args, setup), (_, args2, _) in zip(cases(H, np.random.default_rng(A.HIP_SEED), True), second):
            t0 = time.perf_counter()
            refs, teardown = setup() if setup else (None, lambda: None)
            line = {"entry": name}
            try:
                want1, want2 = A.check_stream_contract(getattr(H.lib, "ivit_" + name), H, args, args2, mem, refs, "ivit_" + name, eager_first=False)
                if any(np.array_equal(a, b) for a, b in zip(want1, want2)):
                    raise A.ContractError(f"ivit_{name}: the second inputs give the first outputs: step 5 proves nothing")
                if name == "layernorm":
                    want = A.ln_lds_case(2056)[3]
                    if not np.array_equal(want1[0], want.view(np.uint8).reshape(-1)):
                        raise A.ContractError("ivit_layernorm: the replay differs from the oracle")
                line["ok"] = True
            except A.ContractError as e:
                line["error"], ok = str(e), False
            finally:
                teardown()
            line["seconds"] = round(time.perf_counter() - t0, 3)
            print(json.dumps(line), flush=True)
            if not ok:
                break
        H.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
