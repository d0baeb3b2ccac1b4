"""Both sides of every 32-bit size limit in the launchers: the table of size decisions, the case table that
tests/test_large_sizes_cpu.py (arithmetic, no device) and tests/test_large_sizes_gpu.py (one launch per case on the device) share, the
predicates of csrc/ivit_hip.hip and csrc/ivit_model.h restated in Python next to their file:line, and the repeat / compare helpers.

How a multi-GB output is checked byte for byte with nothing large on the host: every operator here is independent per row (per image
for the scatters, the attentions and the patch embedding), so a case builds a block of `period` rows (images) on the host — a period
that is no multiple of a kernel's tile — computes the CPU oracle's answer for the block, repeats the block on the device up to M rows
(`repeat_rows`: the last repeat is cut at M) and compares the whole output with the oracle block repeated (`first_mismatch`: pieces of
at most CHUNK_BYTES, each piece against a stride-0 view of the block, every byte, the first differing row reported).

THE TABLE OF SIZE DECISIONS (hip = i-vit_amd/csrc/ivit_hip.hip, model = i-vit_amd/csrc/ivit_model.h; "near | far" = the two sizes a
case pair runs and what happens at each; a kernel name is the one the launcher's code picks)

 file:line        predicate / cast relied on                      near | far                                   what happens
 ---------------- ----------------------------------------------- -------------------------------------------- -----------------------------------
 hip:855-862      launch_gemm3 astat: out_bytes < 2^31            16 bit, N 1536, K 384: M 699050 | 699051     gemm_as_kernel | gemm_ps_kernel
   (out_bytes = M * ldc * (1 | 2); qkv: max(M * D,                residual, N 512: M 2097151 | 2097152         gemm_as_kernel | gemm_ps_kernel
    (M / T + 1) * D * ldv))                                       qkv D 384, T 195: B 28679 | 28680            gemm_as_kernel | gemm_ps_kernel
                                                                    (M 5592405 = 28679 * 195 is the issue's last size below the
                                                                     limit; 5592406 = 2 * 2796203 is not a whole number of images of
                                                                     a usable T: the far side is the next image, M 5592600)
                                                                  qkv v^T, B 2: ldv 1864128 | 1864144          gemm_as_kernel | gemm_ps_kernel
 hip:858          launch_gemm3 astat: M * lda < 2^32              8 bit, N 32, K 384: M 11184810 | 11184811    gemm_as_kernel | gemm_ps_kernel
 hip:858          launch_gemm3 astat: N * ldb < 2^32              left out: weights of 4 GiB; arithmetic only
 gemm3.h:123      ga_rsrc num_records 0x7ffffff0, GA_OOB 2^31     covered by the out_bytes pairs: the largest in-range store ends at
 gemm3.h:781-887                                                  out_bytes <= 2^31 - 16 = num_records (ldc % 16 == 0); dead lanes at 2^31
 gemm3.h:793      bh = b * H + head in unsigned                   B * H < 2^31 / (T * dh) under out_bytes < 2^31: the qkv pairs
 hip:974          qkv on launch_gemm3 only while B * T < 2^23     D 320, T 256: B 32767 | 32768                gemm_ps_kernel | gemm_glds_kernel<EPI_QKV>
   (g3_div: float reciprocal, operands < 2^23)
 hip:772          ws_plan_ok: M < 2^26                            left out: 12.9 GB of input alone; arithmetic only
 hip:774          qkv_ws_ok: B * H * T * 64 < 2^31                K 192, H 3, T 197: B 56775 | 56776           gemm_ws_qkv_kernel | plain:
   (gemm_ws.h:151 per-token offsets are int)                       with and without norm1                      gemm_glds_kernel<EPI_QKV>, norm1
                                                                                                               form: IVIT_ERR_UNSUPPORTED
 hip:775          qkv_ws_ok: B * T < 2^26                         left out: implied by hip:774 (B * T * 64 >= 2^32 there); arithmetic only
 hip:777          qkv_ws_ok: B * H * 64 * ldv < 2^31              B 1024: ldv 10912 | 10928                    gemm_ws_qkv_kernel<VT> | plain:
   (gemm_ws.h:152)                                                 with and without norm1                      gemm_glds_kernel<EPI_QKV>, norm1
                                                                                                               form: IVIT_ERR_UNSUPPORTED
 hip:950          residual + LayerNorm form: M < 2^26             left out (arithmetic only); the entry runs once past 2^31 bytes
 hip:350          launch_gemm: nb <= 65535 (gridDim.y)            ivit_attn_qk_requant BH 65535 | 65536        gemm_nt_kernel | IVIT_ERR_UNSUPPORTED
                                                                   (also ivit_bmm_nt_*, ivit_attn_pv_requant)
 hip:356          launch_gemm grid (unsigned)(tm * tiles_n)       int product: "does not fit an int", left out
 hip:1919         ivit_im2col_patch: B <= 65535                   B 65535 | 65536 (16 x 16, P 16, Cin 3)       im2col_patch16_kernel | im2col_patch_kernel
 hip:1925         (unsigned)(B * (H / P)): an int product         65536 * 1: the far case above; beyond int: left out
 hip:1933         ivit_embed_finish: B <= 65535                   B 65535 | 65536                              embed_finish_kernel | IVIT_ERR_INVALID
 hip:1933,1956    T * D / 8 < 2^22                                left out: a model with 4 M 16-byte pieces per image; arithmetic only
 hip:1955         ivit_patch_embed: B * np < 2^30                 left out (B <= 65535 first unless np >= 16385); arithmetic only
 hip:1956         ivit_patch_embed: B <= 65535                    B 65535 | 65536                              gemm_glds_kernel<.., IM2COL> |
                                                                                                               IVIT_ERR_UNSUPPORTED
 hip:2338         ivit_hidden_f32: gy = min(batch, 65535)         batch 70001 (past), both layouts             hidden_f32_kernel strides over images
 hip:2324         ivit_hidden_f32: batch, rows fit an int         left out ("does not fit an int")
 hip:2345         ivit_hidden_f32: gx = min(.., 2^20)             left out: beyond 2^28 pieces per image
 model:402,894    run_slices: images per slice <= 65535           micro_vit and a patch-16 config: 65535 | 65536  forward | IVIT_ERR_UNSUPPORTED,
   (65535 / heads without the fused attention)                     in one slice; 65536 in two slices            "images per slice"; two slices run
                                                                  2 heads of 32 (no fused attention): 32767 | 32768 in one slice, the same
 model:632-695    (int)M of a Swin slice                          left out ("does not fit an int")
 hip:225-231      grid_for: int after a cap of 16 * num_cu        requant / quantize / widen cases (grid-stride loops in long long)
 elementwise.h:14-16   quantize_input_kernel (long long i)        n = 2^31 + 4099 (past)                       quantize_input_kernel
 elementwise.h:157-169 requant_kernel (long long i, i % C)        2^30 + 4099 elements, C 1 (past)             requant_kernel<int32_t, 8>
 elementwise.h:183-207 requant_vec8_kernel (i * 8 long long)      2^30 + 4104 elements, C 8 (past: a multiple  requant_vec8_kernel<int32_t, 16>
                                                                   of 8 is what the form takes)
 swin.h:663       widen_i8_i16_kernel (long long i)               n = 2^31 + 4099 (past)                       widen_i8_i16_kernel
 hip:1691, layernorm.h:297-316 layernorm_reg_kernel (long long row) C 384: 5596505 rows (past)                 layernorm_reg_kernel<384, 2>
 hip:1823, swin.h:245-329 layernorm_tokenorder8_kernel (gr * CC)  C 96, 49 tokens: 456529 images (past)        layernorm_tokenorder8_kernel<1, 96>
 hip:1653-1666, elementwise.h:683-724 shiftgelu_lut2_kernel       C 1536: 1402201 rows (past)                  shiftgelu_lut2_kernel<3>
   (row * C; a launch holds fewer than 2^32 work-items: the       C 16: 134221828 rows, 16777729 blocks of     shiftgelu_lut2_kernel<1>, in launches
    runtime takes blocks x threads modulo 2^32, no error)          256 threads in all (past)                    of 2^25 rows (2^22 blocks) each
 hip:120-129      launch_fits: blocks x threads < 2^32, at every  ivit_shiftmax n 17: rows 67108860 | 67108861 shiftmax_kernel | IVIT_ERR_UNSUPPORTED
   launcher whose grid is (rows + k - 1) / k: shiftmax (masked),  ivit_layernorm C 8: 134217720 | 134217721    layernorm_kernel<false> | IVIT_ERR_UNSUPPORTED
   shiftgelu, the LayerNorms, token-order, top-k, score,          ivit_logits_topk 2 classes: batch 67108861   IVIT_ERR_UNSUPPORTED (far side only)
   features, cls-probs, class map, attention (B * H blocks of     ivit_layernorm_requant: 2^29 - 32 rows at its narrowest dispatched width is 103 GB of
   512), gather_rows, the generic im2col, the debug kernels       input (17 GB at C = 8 on layernorm16_kernel): left out, arithmetic only (LEFT_OUT)
 hip:1659         shiftgelu_lut_kernel (iter > 6: C > 3072)       left out: no model has the width; same row * C cast
 hip:1545, elementwise.h:421-443 shiftmax_kernel (row * ld)       n 197: 10905033 rows, 8 and 16 bit (past)    shiftmax_kernel
 hip:1611,1626    shiftgelu_kernel (row * C)                      left out: the table kernels are the ones the models run
 hip:356, gemm.h:96-290 gemm_nt_kernel ((long long)grow * ldc)    K 48, N 64, 8 bit: M 33555464 (past)         gemm_nt_kernel<false, EPI_RQ8_CH>
 hip:368-372, gemm2.h:95-294 gemm_glds_kernel                     K 64, N 64, 16 bit: M 33555464 (past)        gemm_glds_kernel<EPI_RQ16_CH, *>
 hip:403, gemm_wreg.h:86-170 gemm_wreg_kernel (row * ldc)         residual, K 192, N 192: M 11185843 (past)    gemm_wreg_kernel<EPI_RQ16_CH_RES, 6, 3>
 hip:783, gemm_ws.h:133-272 gemm_ws_qkv_kernel, plain rows        norm1 + 8-bit layer K 192, N 64: M 11185843  gemm_ws_qkv_kernel<Ws192Geo, .., LN, RQ8>
                                                                  residual + norm2, 384: M 2797235 (past 2^31  gemm_ws_qkv_kernel<Ws384Geo, .., LN, RES16>
                                                                   bytes; 2^32 needs 12.9 GB)
 hip:1264, attention.h:99-108,518 attn_fused_kernel (bh * T * 64) H 3, T 197: B 56776 (past)                   attn_fused_kernel<4, true, 197>
 hip:2051, swin.h:413-468,627 window_attention_kernel (tok_off)   R 56, heads 3, shift 0 and 3: B 2378 (past)  window_attention_kernel<false>
 hip:2048         window_attention_kernel<true> (tables)          left out: the same tok_off, chosen by tables not by size
 hip:2005         window_attention12_kernel                       left out: window 12 is not in the issue's list
 hip:1149, mlp.h:173-187, mlp_body.h:39,313,353 mlp192_kernel     width 192: M 11185843 (past)                 mlp192_kernel
 hip:1163         mlp384_kernel / mlp384rs_kernel grids           left out: min(units, CUs), the same body in long long
 hip:1205         mlp128_kernel                                   left out: the same body
 hip:2100, swin_mlp_rs.h:71-223, swin.h:733-867 swin Mlp          width 96: M 22370654 (past)                  swin_mlp_rs_kernel
 hip:301-320      pil_eval: B * ceil(crop / 32) * 512 < 2^32      left out: 2^23 images of a host descriptor table; arithmetic only
 hip:1466         ivit_gather_rows_i16: n < 2^39, launch_fits     left out: 2^32 pieces of 16 bytes
 hip:1805,1815    avgpool: (unsigned)(B * C + 255), int product   left out ("does not fit an int")
 hip:1896,1905    debug kernels                                   left out: diagnostics
 hip:2148-2304    top-k / score / features / cls-probs / class    one wavefront per row, 4 per block: blocks x 256 < 2^32 from 2^26 - 3 rows
                  map grids                                       (launch_fits above); B * H and batch * k beyond an int: left out
 hip:2363-2444    gallery search: min(.., 2^20), splits <= 65535, left out: pinned by tests/test_search_gpu.py at their own sizes
   index_base + rows <= 2^31 - 1

Deliberately left out of the device runs, one line each (the CPU test holds their two sides to the table by arithmetic, LEFT_OUT):
 ws_plan_ok M < 2^26 — 12.9 GB of input alone.   qkv_ws_ok B * T < 2^26 — the same rows.   ivit_patch_embed B * np >= 2^30 — 2^30 patch
 rows.   ivit_hidden_f32 beyond 2^28 pieces per image — 4 GiB per image.   every "does not fit an int" limit on B * H or batch * k —
 more rows than the device holds.   N * ldb < 2^32 — 4 GiB of weights.
"""
import numpy as np

GIB = 1 << 30
CAP_BYTES = 12 * GIB                # no case holds more on the device at once
CHUNK_BYTES = 256 << 20             # a compared piece
GUARD_BYTES, FILL = 4096, 0x5A      # as guarded() of tests/test_search_gpu.py
COMPARE_BYTES = 3 * CHUNK_BYTES     # what a comparison holds beside the arrays: the piece's mask and, after a difference, its copy
P_ROWS = 4099                       # rows of a block: a prime
P_GEMM = 1031                       # rows of a GEMM block (the oracle multiplies it on the CPU): a prime


# ---------------------------------------------------------------- repeat and compare, on numpy or on torch
def _is_np(xp):
    return xp is np


def _like(a):
    return {} if isinstance(a, np.ndarray) else {"device": a.device}


def repeat_rows(xp, block, M):
    """[M, ...] whose row r is block[r % p], p = block.shape[0]: whole repeats by one broadcast store, the last one cut at M"""
    p, rest = block.shape[0], tuple(block.shape[1:])
    out = xp.empty((M,) + rest, dtype=block.dtype, **_like(block))
    full = M // p
    if full:
        out[:full * p].reshape((full, p) + rest)[...] = block
    if M - full * p:
        out[full * p:] = block[:M - full * p]
    return out


def _equal(xp, a, b):
    return bool(np.array_equal(a, b)) if _is_np(xp) else bool(xp.equal(a, b))


def _first_true(xp, mask):
    flat = mask.reshape(-1)
    return int(np.flatnonzero(flat)[0]) if _is_np(xp) else int(xp.nonzero(flat)[0, 0])


def _periods(xp, flat, k, pe):
    """stride-0 view [k, pe] of the flat block: the expected piece, never materialised"""
    return np.broadcast_to(flat, (k, pe)) if _is_np(xp) else flat.unsqueeze(0).expand(k, pe)


def first_mismatch(xp, got, block, chunk_bytes=CHUNK_BYTES):
    """got [M, ...] against block[r % p] for every row r: None when every element is equal, else the index of the first differing ROW.
    Pieces of at most chunk_bytes (at least one period), each against a view of the block; every element is compared."""
    assert got.dtype == block.dtype and tuple(got.shape[1:]) == tuple(block.shape[1:]), (got.dtype, block.dtype, got.shape, block.shape)
    M, p = got.shape[0], block.shape[0]
    W = 1
    for s in got.shape[1:]:
        W *= int(s)
    gf, bf = got.reshape(-1), block.reshape(-1)
    pe = p * W
    item = got.element_size() if hasattr(got, "element_size") else got.itemsize
    k = max(1, chunk_bytes // (pe * item))
    full = M // p
    for c in range(0, full, k):
        kk = min(k, full - c)
        piece, want = gf[c * pe:(c + kk) * pe].reshape(kk, pe), _periods(xp, bf, kk, pe)
        if not _equal(xp, piece, want):
            return (c * pe + _first_true(xp, piece != want)) // W
    rem = (M - full * p) * W
    if rem and not _equal(xp, gf[full * pe:], bf[:rem]):
        return (full * pe + _first_true(xp, gf[full * pe:] != bf[:rem])) // W
    return None


def all_equal_to(xp, flat, value, chunk_bytes=CHUNK_BYTES):
    """every element of a flat array equals `value` (an untouched output, the pad columns of v^T), piece by piece"""
    item = flat.element_size() if hasattr(flat, "element_size") else flat.itemsize
    n, step = flat.shape[0], max(1, chunk_bytes // item)
    return all(bool((flat[i:i + step] == value).all()) for i in range(0, n, step))


def where_it_is(row, width, item):
    """the text an assertion shows beside a first differing row: where the 2^31 and 2^32 lines lie"""
    return (f"first differing row {row} (width {width} elements of {item} bytes: element offset {row * width}, byte offset {row * width * item}; "
            f"2^31 elements at row {-(-2 ** 31 // width)}, 2^32 bytes at row {-(-2 ** 32 // (width * item))})")


# ---------------------------------------------------------------- the predicates, restated
def use_gemm2(K, lda, ldb):                                     # hip:376
    return K % 32 == 0 and K >= 64 and lda % 16 == 0 and ldb % 16 == 0


def wreg_nct(M, N, K):                                          # hip:380-386 (plain row-major operands)
    if K % 32 or K not in (96, 128, 192) or N % 32 or M < 8192:
        return 0
    nt = N // 32
    return 3 if nt % 3 == 0 else (2 if nt % 2 == 0 else 0)


def use_gemm3(M, N, K, epi_bit, pipelined_ok=True):             # hip:761-768
    if epi_bit == 4 and N < 512:
        return False
    return pipelined_ok and K % 64 == 0 and K >= 320 and N % 16 == 0 and M >= 128


def ws_width(K):                                                # gemm_ws.h:57
    return K in (192, 384)


def ws_plan_ok(prepared, K, M):                                 # hip:772
    return prepared and ws_width(K) and M < (1 << 26)


def qkv_ws_ok(prepared, K, N, B, T, H, dh, ldv=0):              # hip:773-778
    if not (prepared and dh == 64 and ws_width(K) and N == 3 * H * dh and N % 192 == 0 and B * H * T * 64 < (1 << 31) and B * T < (1 << 26)):
        return False
    return ldv == 0 or (K == 192 and ldv >= T and ldv % 16 == 0 and B * H * 64 * ldv < (1 << 31))


def gemm3_out_bytes(epi, M, ldc, D=0, T=0, ldv=0):              # hip:855-856
    if epi == "qkv":
        return max(M * D, (M // (T if T > 0 else 1) + 1) * D * ldv)
    return M * ldc * (1 if epi == "rq8" else 2)


def gemm3_astat(epi, M, N, K, D=0, T=0, dh=0, ldv=0):           # hip:857-860 (lda = ldb = K, ldc = N)
    return (K % 384 == 0 and M >= 256 and N % 32 == 0 and M * K < (1 << 32) and N * K < (1 << 32) and
            gemm3_out_bytes(epi, M, N, D, T, ldv) < (1 << 31) and (epi != "qkv" or (D % 128 == 0 and dh % 32 == 0)))


def qkv_planned_route(prepared, B, T, H, dh, ldv=0):            # hip:973-975: the kernel ivit_linear_i8_qkv_planned picks
    D = H * dh
    if qkv_ws_ok(prepared, D, 3 * D, B, T, H, dh, ldv):
        return "gemm_ws_qkv_kernel"
    if use_gemm3(B * T, 3 * D, D, 2) and B * T < (1 << 23):
        return "gemm_as_kernel" if gemm3_astat("qkv", B * T, 3 * D, D, D, T, dh, ldv) else "gemm_ps_kernel"
    return "gemm_glds_kernel" if use_gemm2(D, D, D) else "gemm_nt_kernel"


def requant_planned_route(prepared, M, N, K, bits):             # hip:891-894
    if bits == 8 and ws_plan_ok(prepared, K, M):
        return "gemm_ws_qkv_kernel"
    if use_gemm3(M, N, K, 1):
        return "gemm_as_kernel" if gemm3_astat("rq8" if bits == 8 else "rq16", M, N, K) else "gemm_ps_kernel"
    return linear_route(M, N, K)


def residual_planned_route(prepared, M, N, K):                  # hip:926-929 (residual multipliers in the fast range)
    if ws_plan_ok(prepared, K, M):
        return "gemm_ws_qkv_kernel"
    if use_gemm3(M, N, K, 4):
        return "gemm_as_kernel" if gemm3_astat("res16", M, N, K) else "gemm_ps_kernel"
    return linear_route(M, N, K)


def linear_route(M, N, K):                                      # hip:448-450, 489-491
    if wreg_nct(M, N, K):
        return "gemm_wreg_kernel"
    return "gemm_glds_kernel" if use_gemm2(K, K, K) else "gemm_nt_kernel"


def im2col_route(B, Cin, W, P):                                 # hip:1919
    return "im2col_patch16_kernel" if P == 16 and Cin == 3 and W % 16 == 0 and B <= 65535 else "im2col_patch_kernel"


def embed_finish_ok(B, T, D):                                   # hip:1933
    return T * D // 8 < (1 << 22) and B <= 65535


def patch_embed_ok(B, np_, T, D, K, P=16):                      # hip:1955-1956 (16 x 16 patches, fast multipliers)
    return P == 16 and D % 8 == 0 and K % 64 == 0 and use_gemm2(K, K, K) and B * np_ < (1 << 30) and T * D // 8 < (1 << 22) and B <= 65535


def batched_ok(nb):                                             # hip:350
    return nb <= 65535


def launch_fits(blocks, threads):                               # hip:120-129
    return blocks * threads < (1 << 32)


def max_slice_images(fused_attention, heads):                   # model:402
    return 65535 if fused_attention else 65535 // heads


def shiftgelu_lut_route(C):                                     # hip:1649-1665
    it = (C // 16 + 31) // 32
    return "shiftgelu_lut_kernel" if it > 6 else "shiftgelu_lut2_kernel<%d>" % (it if it <= 4 else 6)


# ---------------------------------------------------------------- the cases
class Case:
    """one launch: `entry` the C entry (or the runner), `run` the body of tests/test_large_sizes_gpu.py that runs it, `limit` the size
    decision of the table, `side` near / far (a pair, `pair` names it) or past (a kernel without a predicate), `sizes` the shape,
    `period` rows or images of the host block, `kernel` what the launcher's code picks, `arrays` {name: bytes} on the device"""

    def __init__(self, cid, entry, run, limit, side, sizes, period, kernel, arrays, pair=None, step=None):
        self.id, self.entry, self.run, self.limit, self.side, self.sizes = cid, entry, run, limit, side, dict(sizes)
        self.period, self.kernel, self.arrays, self.pair, self.step = period, kernel, dict(arrays), pair, step

    @property
    def bytes(self):
        """device bytes the case needs: its arrays with their guards, and what a comparison holds"""
        return sum(self.arrays.values()) + 2 * GUARD_BYTES * len(self.arrays) + COMPARE_BYTES

    def __repr__(self):
        return self.id


def _pair(stem, entry, run, limit, key, near, far, sizes, period, kernels, arrays, step):
    """the last size on the near side of a limit and the first on the far side: `key` is the size that differs, `step` by how much two
    adjacent sizes differ (one row, one image, 16 columns of ldv)"""
    out = []
    for side, v, kern in (("near", near, kernels[0]), ("far", far, kernels[1])):
        s = dict(sizes, **{key: v})
        out.append(Case(f"{stem}-{side}", entry, run, limit, side, s, period, kern, arrays(s), pair=stem, step=(key, step)))
    return out


def _cases():
    cs = []
    two31, two32 = 1 << 31, 1 << 32

    # ---- planned GEMMs on launch_gemm3 (plans as created: not prepared for the weights-in-registers kernel)
    cs += _pair("planned-rq16-out_bytes", "ivit_linear_i8_requant_planned", "planned_requant", "out_bytes < 2^31", "M", 699050, 699051,
                dict(N=1536, K=384, bits=16), P_GEMM, ("gemm_as_kernel", "gemm_ps_kernel"),
                lambda s: dict(x=s["M"] * s["K"], out=s["M"] * s["N"] * 2), 1)
    cs += _pair("planned-rq8-M_lda", "ivit_linear_i8_requant_planned", "planned_requant", "M * lda < 2^32", "M", 11184810, 11184811,
                dict(N=32, K=384, bits=8), P_GEMM, ("gemm_as_kernel", "gemm_ps_kernel"),
                lambda s: dict(x=s["M"] * s["K"], out=s["M"] * s["N"]), 1)
    cs += _pair("planned-res16-out_bytes", "ivit_linear_i8_requant_residual_planned", "planned_residual", "out_bytes < 2^31", "M", 2097151, 2097152,
                dict(N=512, K=384), P_GEMM, ("gemm_as_kernel", "gemm_ps_kernel"),
                lambda s: dict(x=s["M"] * s["K"], residual=s["M"] * s["N"] * 2, out=s["M"] * s["N"] * 2), 1)
    qkv384 = dict(T=195, H=6, dh=64, ldv=0, prepared=False, ln=False)
    cs += _pair("planned-qkv-out_bytes", "ivit_linear_i8_qkv_planned", "planned_qkv", "out_bytes < 2^31 (qkv scatter)", "B", 28679, 28680,
                qkv384, 5, ("gemm_as_kernel", "gemm_ps_kernel"),
                lambda s: dict(x=s["B"] * s["T"] * 384, q=s["B"] * s["T"] * 384, k=s["B"] * s["T"] * 384, v=s["B"] * s["T"] * 384), 1)
    cs += _pair("planned-qkv-vT-out_bytes", "ivit_linear_i8_qkv_planned", "planned_qkv", "out_bytes < 2^31 (v^T term)", "ldv", 1864128, 1864144,
                dict(qkv384, B=2), 2, ("gemm_as_kernel", "gemm_ps_kernel"),
                lambda s: dict(x=s["B"] * s["T"] * 384, q=s["B"] * s["T"] * 384, k=s["B"] * s["T"] * 384, v=s["B"] * 384 * s["ldv"]), 16)

    # D = 320 (no multiple of 384: gemm_ps_kernel on both sides of out_bytes): the scatter's float-reciprocal divisions take rows < 2^23
    cs += _pair("planned-qkv-BT23", "ivit_linear_i8_qkv_planned", "planned_qkv", "B * T < 2^23", "B", 32767, 32768,
                dict(T=256, H=5, dh=64, ldv=0, prepared=False, ln=False), 5, ("gemm_ps_kernel", "gemm_glds_kernel"),
                lambda s: dict(x=s["B"] * 256 * 320, q=s["B"] * 256 * 320, k=s["B"] * 256 * 320, v=s["B"] * 256 * 320), 1)

    # ---- the weights-in-registers qkv kernel (plans prepared), K = 192, H = 3, T = 197, with and without the norm1 prologue
    ws = dict(T=197, H=3, dh=64, prepared=True)
    for ln in (False, True):
        tag = "ln-qkv" if ln else "qkv"
        entry = "ivit_layernorm_linear_i8_qkv_ldv_planned" if ln else "ivit_linear_i8_qkv_planned"
        far = "IVIT_ERR_UNSUPPORTED" if ln else "gemm_glds_kernel"
        xb = 2 if ln else 1
        cs += _pair(f"ws-{tag}-BHT64", entry, "planned_qkv", "B * H * T * 64 < 2^31", "B", 56775, 56776, dict(ws, ldv=0, ln=ln), 5,
                    ("gemm_ws_qkv_kernel", far),
                    lambda s, xb=xb: dict(x=s["B"] * 197 * 192 * xb, q=s["B"] * 197 * 192, k=s["B"] * 197 * 192, v=s["B"] * 197 * 192), 1)
        cs += _pair(f"ws-{tag}-BH64ldv", entry, "planned_qkv", "B * H * 64 * ldv < 2^31", "ldv", 10912, 10928, dict(ws, B=1024, ln=ln), 5,
                    ("gemm_ws_qkv_kernel", far),
                    lambda s, xb=xb: dict(x=s["B"] * 197 * 192 * xb, q=s["B"] * 197 * 192, k=s["B"] * 197 * 192, v=s["B"] * 192 * s["ldv"]), 16)
    # the two ws-only planned forms: their one size predicate (M < 2^26) is left out; each runs once past a 32-bit line
    M32 = -(-two32 // (192 * 2)) + 1 + P_GEMM                 # the last row's 16-bit byte offset is beyond 2^32 at width 192
    cs.append(Case("ws-ln-requant-past", "ivit_layernorm_linear_i8_requant_planned", "planned_ln_requant", "none (M < 2^26 left out)", "past",
                   dict(M=M32, N=64, K=192), P_GEMM, "gemm_ws_qkv_kernel", dict(x16=M32 * 192 * 2, out=M32 * 64)))
    M31 = -(-two31 // (384 * 2)) + 1 + P_GEMM                 # ... beyond 2^31 bytes at width 384 (2^32 would need 12.9 GB)
    cs.append(Case("ws-res-ln-past", "ivit_linear_i8_requant_residual_layernorm_planned", "planned_residual_ln", "none (M < 2^26 left out)", "past",
                   dict(M=M31, N=384, K=384), P_GEMM, "gemm_ws_qkv_kernel",
                   dict(x=M31 * 384, residual=M31 * 384 * 2, out=M31 * 384 * 2, ln_out8=M31 * 384)))

    # ---- kernels with no predicate: the last row's output offset beyond 2^31 elements (2^32 bytes where an operand is 16 or 32 bit)
    n = (1 << 30) + 4099
    cs.append(Case("requant_i32-scalar", "ivit_requant_i32", "requant_i32", "none", "past", dict(rows=n, C=1, bits=8), P_ROWS,
                   "requant_kernel", dict(z=n * 4, out=n)))
    n8 = ((1 << 30) + 4099 + 7) // 8 * 8
    cs.append(Case("requant_i32-vec8", "ivit_requant_i32", "requant_i32", "none", "past", dict(rows=n8 // 8, C=8, bits=16), P_ROWS,
                   "requant_vec8_kernel", dict(z=n8 * 4, out=n8 * 2)))
    n = two31 + 4099
    cs.append(Case("quantize_input_f32", "ivit_quantize_input_f32", "quantize_input", "none", "past", dict(n=n), P_ROWS,
                   "quantize_input_kernel", dict(x=n * 4, q=n)))
    cs.append(Case("widen_i8_i16", "ivit_widen_i8_i16", "widen", "none", "past", dict(n=n), P_ROWS, "widen_i8_i16_kernel", dict(x=n, out=n * 2)))
    rows = two31 // 384 + 1 + P_ROWS
    cs.append(Case("layernorm_requant-384", "ivit_layernorm_requant", "layernorm_requant", "none", "past", dict(rows=rows, C=384), P_ROWS,
                   "layernorm_reg_kernel<384, 2>", dict(x=rows * 384 * 2, out=rows * 384)))
    B = -(-(two31 // 96 + 2) // 49) + 5                        # images of 49 tokens
    cs.append(Case("layernorm_tokenorder-96", "ivit_layernorm_tokenorder_requant", "layernorm_tokenorder", "none", "past", dict(B=B, L=49, C=96), 5,
                   "layernorm_tokenorder8_kernel<1, 96>", dict(x=B * 49 * 96 * 2, out=B * 49 * 96)))
    rows = two31 // 1536 + 1 + P_ROWS
    cs.append(Case("shiftgelu_lut-1536", "ivit_shiftgelu_requant_lut", "shiftgelu_lut", "none", "past", dict(rows=rows, C=1536), P_ROWS,
                   shiftgelu_lut_route(1536), dict(x=rows * 1536, out=rows * 1536)))
    rows = two31 // 16 + 1 + P_ROWS                           # the narrowest row the entry takes: the largest grid2 = ceil(rows / 8)
    cs.append(Case("shiftgelu_lut-16", "ivit_shiftgelu_requant_lut", "shiftgelu_lut", "none (grid2 largest)", "past", dict(rows=rows, C=16), P_ROWS,
                   shiftgelu_lut_route(16), dict(x=rows * 16, out=rows * 16)))
    rows = two31 // 197 + 2 + P_ROWS                          # odd: the last block of four rows is partial
    for bits in (8, 16):
        cs.append(Case(f"shiftmax-197-{bits}", "ivit_shiftmax", "shiftmax", "none", "past", dict(rows=rows, n=197, bits=bits), 259,
                       "shiftmax_kernel", dict(x=rows * 197, out=rows * 197 * 2)))
    M = two31 // 64 + 1 + P_GEMM
    cs.append(Case("linear_requant-gemm_nt", "ivit_linear_i8_requant", "linear_requant", "none", "past", dict(M=M, N=64, K=48, bits=8), P_GEMM,
                   linear_route(M, 64, 48), dict(x=M * 48, out=M * 64)))
    cs.append(Case("linear_requant-gemm2", "ivit_linear_i8_requant", "linear_requant", "none", "past", dict(M=M, N=64, K=64, bits=16), P_GEMM,
                   linear_route(M, 64, 64), dict(x=M * 64, out=M * 64 * 2)))
    cs.append(Case("linear_residual-wreg", "ivit_linear_i8_requant_residual", "linear_residual", "none", "past", dict(M=M32, N=192, K=192), P_GEMM,
                   linear_route(M32, 192, 192), dict(x=M32 * 192, residual=M32 * 192 * 2, out=M32 * 192 * 2)))
    B = 56776
    cs.append(Case("attention_fused-197", "ivit_attention_fused", "attention", "none", "past", dict(B=B, H=3, T=197, dh=64, ldv=208), 5,
                   "attn_fused_kernel<4, true, 197>", dict(q=B * 3 * 197 * 64, k=B * 3 * 197 * 64, vt=B * 3 * 64 * 208, ctx=B * 197 * 192)))
    B = 2378
    for shift in (0, 3):
        cs.append(Case(f"window_attention-56-shift{shift}", "ivit_window_attention_fused", "window_attention", "none", "past",
                       dict(B=B, R=56, heads=3, shift=shift), 3, "window_attention_kernel<false>",
                       dict(qkv=B * 56 * 56 * 288, ctx=B * 56 * 56 * 96)))
    cs.append(Case("mlp_fused_planned-192", "ivit_mlp_fused_planned", "mlp_planned", "none", "past", dict(M=M32, C=192), P_GEMM, "mlp192_kernel",
                   dict(x=M32 * 192, residual=M32 * 192 * 2, out=M32 * 192 * 2)))
    M96 = -(-two32 // (96 * 2)) + 1 + P_GEMM
    cs.append(Case("swin_mlp_fused-96", "ivit_mlp_fused", "mlp_swin", "none", "past", dict(M=M96, C=96), P_GEMM, "swin_mlp_rs_kernel",
                   dict(x=M96 * 96, residual=M96 * 96 * 2, out=M96 * 96 * 2)))

    # ---- the 65535 limit of gridDim.y: megabytes
    img = 3 * 16 * 16
    cs += _pair("im2col-B", "ivit_im2col_patch", "im2col", "B <= 65535", "B", 65535, 65536, dict(Cin=3, HW=16, P=16), 7,
                ("im2col_patch16_kernel", "im2col_patch_kernel"), lambda s: dict(img=s["B"] * img, rows=s["B"] * img), 1)
    pe = dict(Cin=3, HW=16, P=16, D=64)
    cs += _pair("patch_embed-B", "ivit_patch_embed", "patch_embed", "B <= 65535", "B", 65535, 65536, pe, 7,
                ("gemm_glds_kernel<EPI_RQ16_CH_RES, 128, IM2COL>", "IVIT_ERR_UNSUPPORTED"),
                lambda s: dict(img=s["B"] * img, x16=s["B"] * 2 * 64 * 2, rows=s["B"] * img, patch16=s["B"] * 64 * 2, chain=s["B"] * 2 * 64 * 2), 1)
    cs += _pair("embed_finish-B", "ivit_embed_finish", "embed_finish", "B <= 65535", "B", 65535, 65536, dict(T=2, D=64), 7,
                ("embed_finish_kernel", "IVIT_ERR_INVALID"), lambda s: dict(patch16=s["B"] * 64 * 2, x16=s["B"] * 2 * 64 * 2), 1)
    cs += _pair("attn_qk-BH", "ivit_attn_qk_requant", "attn_qk", "nb <= 65535", "BH", 65535, 65536, dict(T=5, dh=16, lds=16), 7,
                ("gemm_nt_kernel<false, EPI_RQ8_S>", "IVIT_ERR_UNSUPPORTED"),
                lambda s: dict(q=s["BH"] * 5 * 16, k=s["BH"] * 5 * 16, scores=s["BH"] * 5 * 16), 1)
    # ---- a launch holds fewer than 2^32 work-items: the last row count a row-per-wavefront launcher takes, and the first it refuses
    top = ((1 << 24) - 1) * 4                                 # 4 rows per block of 256 threads
    cs += _pair("shiftmax-work_items", "ivit_shiftmax", "shiftmax_limit", "blocks * threads < 2^32", "rows", top, top + 1, dict(n=17, bits=16), 259,
                ("shiftmax_kernel", "IVIT_ERR_UNSUPPORTED"), lambda s: dict(x=s["rows"] * 17, out=s["rows"] * 17 * 2), 1)
    top8 = ((1 << 24) - 1) * 8                                # 8 rows per block of 256 threads
    cs += _pair("layernorm-work_items", "ivit_layernorm", "layernorm_limit", "blocks * threads < 2^32", "rows", top8, top8 + 1, dict(C=8), P_ROWS,
                ("layernorm_kernel<false>", "IVIT_ERR_UNSUPPORTED"), lambda s: dict(x=s["rows"] * 8 * 2, z=s["rows"] * 8 * 4), 1)
    cs.append(Case("logits_topk-work_items-far", "ivit_logits_topk", "topk_limit", "blocks * threads < 2^32", "far", dict(batch=top + 1, ncls=2, k=1), 1,
                   "IVIT_ERR_UNSUPPORTED", dict(logits=(top + 1) * 8, idx=(top + 1) * 4, val=(top + 1) * 4)))
    for layout in ("tokens", "grid"):
        cs.append(Case(f"hidden_f32-{layout}", "ivit_hidden_f32", "hidden_f32", "gy = min(batch, 65535)", "past",
                       dict(batch=70001, T=3, C=8, t0=1, layout=layout), 7, "hidden_f32_kernel<%s>" % ("true" if layout == "grid" else "false"),
                       dict(x16=70001 * 3 * 8 * 2, out=70001 * 2 * 8 * 4)))
    # the ViT runner: a self-calibrated patch-16 config (one PatchEmbed launch) and micro_vit (patch 8: im2col -> GEMM -> embed_finish)
    for model, lim in (("patch16", 65535), ("micro_vit", 65535), ("patch16h2", 32767)):
        cs.append(Case(f"runner-{model}-{lim}", "ivit_vit_forward", "runner", f"images per slice <= {lim}", "near",
                       dict(model=model, batch=lim, nslices=1, limit=lim), 7, "forward", dict(), pair=f"runner-{model}", step=("batch", 1)))
        cs.append(Case(f"runner-{model}-{lim + 1}", "ivit_vit_forward", "runner", f"images per slice <= {lim}", "far",
                       dict(model=model, batch=lim + 1, nslices=1, limit=lim), 7, "IVIT_ERR_UNSUPPORTED", dict(), pair=f"runner-{model}", step=("batch", 1)))
        cs.append(Case(f"runner-{model}-{lim + 1}-two-slices", "ivit_vit_forward", "runner", f"images per slice <= {lim}", "near",
                       dict(model=model, batch=lim + 1, nslices=2, limit=lim), 7, "forward", dict()))
    return cs


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# the runner configs: (img, patch, embed_dim, depth, heads, classes); the workspace of a slice is asked of the library at run time and
# held to the cap there, these are the bytes a case states for the CPU test (images + logits + a bound on the workspace per image)
RUNNER_MODELS = {"patch16": dict(img=32, patch=16, D=64, depth=1, heads=1, ncls=5), "micro_vit": None,
                 "patch16h2": dict(img=32, patch=16, D=64, depth=1, heads=2, ncls=5)}       # 2 heads of 32: the unfused attention chain
RUNNER_WS_PER_IMAGE = 64 * 1024
for _c in CASES:
    if _c.run == "runner":
        _b = _c.sizes["batch"]
        _c.arrays.update(images=_b * 3 * 32 * 32, workspace=_b * RUNNER_WS_PER_IMAGE, logits=2 * _b * 10 * 4)


def ids(run):
    return [c.id for c in CASES if c.run == run]


# every entry the issue names, and the limits left to arithmetic
ENTRIES_NAMED = (
    "ivit_linear_i8_requant_planned", "ivit_layernorm_linear_i8_requant_planned", "ivit_linear_i8_requant_residual_planned",
    "ivit_linear_i8_requant_residual_layernorm_planned", "ivit_linear_i8_qkv_planned", "ivit_layernorm_linear_i8_qkv_ldv_planned",
    "ivit_requant_i32", "ivit_quantize_input_f32", "ivit_widen_i8_i16", "ivit_layernorm_requant", "ivit_layernorm_tokenorder_requant",
    "ivit_shiftgelu_requant_lut", "ivit_shiftmax", "ivit_linear_i8_requant", "ivit_linear_i8_requant_residual", "ivit_attention_fused",
    "ivit_window_attention_fused", "ivit_mlp_fused_planned", "ivit_mlp_fused", "ivit_im2col_patch", "ivit_patch_embed", "ivit_embed_finish",
    "ivit_hidden_f32", "ivit_vit_forward", "ivit_layernorm", "ivit_logits_topk")

# (name, predicate of the size, last size inside, first size outside): held to the table by arithmetic only
LEFT_OUT = (
    ("ws_plan_ok: M < 2^26", lambda M: ws_plan_ok(True, 384, M), (1 << 26) - 1, 1 << 26),
    # (the term alone: with H >= 1 it is implied by B * H * T * 64 < 2^31 of the line above it, so no size reaches it)
    ("qkv_ws_ok: B * T < 2^26", lambda BT: BT < (1 << 26), (1 << 26) - 1, 1 << 26),
    ("ivit_patch_embed: B * np < 2^30 (np = 16384)", lambda B: patch_embed_ok(B, 16384, 16385, 8, 768), 65535, 65536),
    ("ivit_patch_embed: T * D / 8 < 2^22 (D = 8)", lambda T: patch_embed_ok(1, T - 1, T, 8, 768), (1 << 22) - 1, 1 << 22),
    ("ivit_hidden_f32: 2^20 blocks of 256 pieces cover an image", lambda per: (per + 255) // 256 <= (1 << 20), 1 << 28, (1 << 28) + 1),
    ("does not fit an int: B * H, batch * k (behind the 2^32 work-items of their launches)", lambda n: n <= 0x7fffffff, (1 << 31) - 1, 1 << 31),
    ("launch_gemm3: N * ldb < 2^32 (K = 384)", lambda N: N * 384 < (1 << 32), 11184810, 11184811),
    ("4 rows per 256-thread block (shiftgelu, score, features, cls-probs, class map)", lambda rows: launch_fits((rows + 3) // 4, 256), (1 << 26) - 4, (1 << 26) - 3),
    ("ivit_layernorm_requant, C = 96 .. 384: 32 rows per 256-thread block", lambda rows: launch_fits((rows + 31) // 32, 256), (1 << 29) - 32, (1 << 29) - 31),
    ("ivit_layernorm_requant, C = 512 .. 1536: 32 rows per 512-thread block", lambda rows: launch_fits((rows + 31) // 32, 512), (1 << 28) - 32, (1 << 28) - 31),
    ("token-order LayerNorms: 32 rows per 256-thread block", lambda rows: launch_fits((rows + 31) // 32, 256), (1 << 29) - 32, (1 << 29) - 31),
    ("fused attention: one (image, head) per 512-thread block", lambda bh: launch_fits(bh, 512), (1 << 23) - 1, 1 << 23),
    ("pil_eval: one band of an image per 512-thread block", lambda nb: launch_fits(nb, 512), (1 << 23) - 1, 1 << 23),
    ("ivit_shiftgelu_requant_lut: a launch of 2^25 rows is 2^22 blocks", lambda nr: nr <= (1 << 25) and (nr + 7) // 8 * 256 < (1 << 32), 1 << 25, (1 << 25) + 1),
)
