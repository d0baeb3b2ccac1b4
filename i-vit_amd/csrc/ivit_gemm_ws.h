// ivit_gemm_ws.h — the qkv QuantLinear of a D = 384 block (models/vit_quant.py:65-74 through quant_modules.py:21-80) with the
// tokens of a whole CU in LDS and the WEIGHTS of a 64-channel slab in registers — and, optionally, norm1 + qact1
// (quant_modules.py:353-386, quant_utils.py:213-253) computed straight into that LDS image, so that the 8-bit activations of the
// block's first LayerNorm never exist in HBM (vit_quant.py:136-140: norm1's output has one consumer, attn.qkv).
//
//   * a workgroup (8 waves, one per CU) owns a contiguous range of 32-token tiles (<= WS_MAXT per panel: 7 x 32 x 384 B = 86 KB),
//     laid out [64-column block][token][64 B] with the chunk permutation wa_g of ivit_wa.h (conflict-free ds_read_b128
//     B fragments).  LN = false: filled by DMA from the 8-bit activations.  LN = true: every wave normalises 8 rows at a time
//     (ivit_layernorm.h::LnGroup<384, 2>, the same arithmetic as layernorm_reg_kernel, byte for byte) and writes the bytes there;
//   * a wave's task is (64-channel slab = one head of q, k or v; one half of the panel's token tiles): the 2 x 12 16-byte A
//     fragments of the slab (24 KB, rows placed so that accumulator register v of lane (token, h) is channel 16 h + v) are
//     loaded into 96 registers, then the wave sweeps its token tiles two at a time — v_mfma_i32_32x32x32_i8, tokens as the B
//     operand, each B fragment feeding two MFMAs (with one channel tile per wave the LDS read port is the bound: 4 SIMDs x 1 KB
//     per 32-cycle MFMA is its whole 128 B/clk) — and requantises each sweep: fp64 FMA with the magic constant, saturating packs,
//     one 16-byte store per (token, 16 channels);
//   * no workgroup barrier after the prologue; bias and multipliers in LDS, so that the steady state has no vector-memory LOAD
//     behind a store (loads and stores retire through one in-order counter on this chip: a wait for a load is a wait for every
//     store in front of it).
//
// Measured stand-alone at DeiT-S b256: profiles/README.md, round 6.
//
// The text above is the K = 384 geometry (Ws384Geo).  The same source at K = 192 (Ws192Geo: DeiT-Tiny, Swin stage 1): 6 k-steps, 3 K blocks,
// 48 weight registers per slab, 14 tiles per panel swept in pairs by a loop, and — for layers whose attention reads v^T — a second store form
// of the qkv epilogue (VT).  Measured: profiles/README.md, "Width 192 on the weights-in-registers GEMM".
#pragma once
#include "ivit_layernorm.h"
#include "ivit_wa.h"
#include <type_traits>

// One source, two widths.  K = 384: 7 tiles x 32 tokens x 384 B = 86 KB per panel, 96 weight registers per slab.  K = 192: a tile is
// 6 KB and a slab 48 registers; the LDS that frees goes to a panel twice as long (14 tiles, the same 86 KB: a CU that owns more than
// 7 tiles — Swin stage 1 at large batch — passes half as many panel barriers), the registers stay free (the sweep is two token tiles
// as at 384: at four, EPI_RES16's identity rows alone are 64 registers).  VT: the geometry also builds the v^T store form of the
// qkv epilogue, which keeps a second per-token offset table behind the LayerNorm constants
template <int K_, int MAXT_, bool VT_>
struct WsGeo {
    static constexpr int K = K_;
    static constexpr int KS = K_ / 32;                  // k-steps of 32
    static constexpr int KB = K_ / 64;                  // K blocks of 64 columns
    static constexpr int MAXT = MAXT_;                  // 32-token tiles of a panel in LDS
    static constexpr int TOK = MAXT * 32;
    static constexpr int KBLK = TOK * 64;
    static constexpr int SOFF = KB * KBLK;              // output row offset of each token of the panel (int)
    static constexpr int SBIAS = SOFF + TOK * 4;        // the layer's bias (int32 x N) and multipliers (double x N)
    static constexpr int MAXN = 1536;
    static constexpr int SCQ = SBIAS + MAXN * 4;
    static constexpr int SLN = SCQ + MAXN * 8;          // LayerNorm's per-channel constants: c (double), bias_int, sc, 1 / sc (float) x K
    static constexpr int SVOFF = SLN + K * 20;          // v^T form: offset of each token's column in its image's v^T (int)
    static constexpr bool VT = VT_;
    static constexpr int SMEM = SVOFF + (VT ? TOK * 4 : 0);
    static_assert(K % 64 == 0 && TOK <= 512 && KBLK % 256 == 0, "whole K blocks; one thread per token of a panel; K blocks a whole number of bank periods apart");
    static_assert(SMEM <= 160 * 1024, "one workgroup per CU");
};
typedef WsGeo<384, 7, false> Ws384Geo;
typedef WsGeo<192, 14, true> Ws192Geo;
#define WS_MAXN 1536
inline bool ws_width(int K) { return K == Ws384Geo::K || K == Ws192Geo::K; }
#define WS_THREADS 512

struct WsArgs {
    const int8_t *x;          // [M][K] 8-bit activations (LN = false)
    const v4i *wf;            // swizzled weights: fragment (ct * (K / 32) + ks) * 64 + lane
    const int32_t *bias;      // [N]
    const double *cq;         // [N]
    int8_t *q, *k, *v;        // [B*H][T][64] each
    int M, N, T, H;
    void *dummy;              // >= 1 KB: where the lanes of rows >= M store
    // LN = true: the block's 16-bit input and norm1's constants (the arguments of ivit_layernorm_requant)
    const int16_t *x16;
    float ln_s;
    int ldv;                  // EPI_QKV8 with VT = true: v is v^T [B*H][64][ldv], element (b, h, t, ch) at ((b * H + h) * 64 + ch) * ldv + t
    const float *ln_bias_int, *ln_sc;
    const ivit_dyadic *ln_dy;
    // EPI = WS_EPI_RES16 (attn.proj + qact2 with the identity branch, vit_quant.py:137-138 + quant_utils.py:238-244): out16 [M][N]
    // = clamp16(rq(residual, cr) + rq(clamp16(rq(acc + bias, cq)), cm)); cm, cr = m * 2^-e of the two dyadic multipliers, |.| < 2^9
    const int16_t *residual;
    int16_t *out16;
    double cm, cr;
    int8_t *ln_out8;          // EPI_RES16 with LN = true: norm2 + qact3 of out16's rows (ln_s .. ln_dy are norm2's), [M][384]
};
#define WS_EPI_QKV8 0
#define WS_EPI_RES16 1
#define WS_EPI_RQ8 2                             // plain QuantLinear -> QuantAct(8): q = out8 [M][N] row-major (Swin's qkv layer)

// weights [N][K] -> fragments of 64 lanes x 16 B: fragment ct * (K / 32) + ks, lane l = (row l & 31, k half l >> 5)
__global__ __launch_bounds__(256) void ws_swizzle_kernel(const int8_t *__restrict__ w, v4i *__restrict__ wf, int N, int K) {
    const int nks = K / 32, nfrag = N / 32 * nks;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nfrag * 64; i += gridDim.x * 256) {
        const int l = i & 63, f = i >> 6, ct = f / nks, ks = f - ct * nks;
        const int ch = 32 * ct + wa_chan_of_row(l & 31);
        wf[i] = *reinterpret_cast<const v4i *>(w + (size_t)ch * K + 32 * ks + 16 * (l >> 5));
    }
}

template <class G, bool FMA, bool LN, int EPI = WS_EPI_QKV8, bool VT = false>
__global__ __launch_bounds__(WS_THREADS, 2) void gemm_ws_qkv_kernel(WsArgs p) {
    static_assert(!VT || (G::VT && EPI == WS_EPI_QKV8), "the v^T store form belongs to the qkv scatter of a geometry that keeps its table");
    static_assert(!(LN && EPI == WS_EPI_RES16) || G::K == 384, "norm2 in the proj launch is built at 384 only");
    extern __shared__ __attribute__((aligned(256))) char sm[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned sm_lds = (unsigned)(size_t)(lds_c *)sm;
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, tok = lane & 31, kh = lane >> 5, e = kh ^ wa_g(tok);

    const int ntt = (p.M + 31) >> 5;
    const int t_beg = (int)((long long)ntt * blockIdx.x / gridDim.x), t_end = (int)((long long)ntt * (blockIdx.x + 1) / gridDim.x);
    const int ncp = p.N >> 6, ncp3 = ncp / 3;                 // 64-channel slabs; per q | k | v
    for (int i = tid; i < p.N; i += WS_THREADS) {
        reinterpret_cast<int *>(sm + G::SBIAS)[i] = p.bias[i];
        reinterpret_cast<double *>(sm + G::SCQ)[i] = p.cq[i];
    }
    const unsigned lane16 = lane * 16;
    double *cC = reinterpret_cast<double *>(sm + G::SLN);
    float *cB = reinterpret_cast<float *>(sm + G::SLN + G::K * 8), *cSc = cB + G::K, *cY = cSc + G::K;
    bool ln_fast = false;
    constexpr bool LN_HEAD = LN && EPI != WS_EPI_RES16, LN_TAIL = LN && EPI == WS_EPI_RES16;
    if constexpr (LN) ln_fast = ln_stage_constants<G::K, WS_THREADS>(p.ln_bias_int, p.ln_sc, p.ln_dy, cC, cB, cSc, cY);

    for (int t0 = t_beg; t0 < t_end; t0 += G::MAXT) {
        const int n_own = min(G::MAXT, t_end - t0);
        if (t0 != t_beg) __syncthreads();            // a later panel: every wave is done with the previous one
        if constexpr (LN_HEAD) {
            // ---- norm1 + qact1 of the panel's rows into the LDS image: 8 rows per wave and pass, 8 lanes per row, lane (k, h)
            // owns channels 32 i + 8 k + 4 h .. + 3 of every step i — 4 bytes of chunk (i & 1) * 2 + (k >> 1) of K block i >> 1
            typedef LnGroup<G::K, 2> LG;
            const int j = lane & 7, k = j >> 1, hh = j & 1;
            const float ys = rcp_rn(p.ln_s);
            // (the phase is VALU-issue-bound like layernorm_reg_kernel itself: requesting pass n + 1's rows ahead, or two rows per lane
            // group for more independent chains, measured 53.5 / 54.4 us against 51.3 for this form)
            for (int r0 = wave * 8; r0 < n_own * 32; r0 += 64) {
                const int tokl = r0 + (lane >> 3);
                const long long row_raw = (long long)t0 * 32 + tokl;
                const bool live = row_raw < p.M;
                const int16_t *xp = p.x16 + (live ? row_raw : (long long)p.M - 1) * G::K + 8 * k + 4 * hh;
                float xv[LG::NSTEP][LG::EPC];
                LN_ROW_X(LG, xv, LG::raw_at(xp + 32 * i), p.ln_s, ys);
                const unsigned rowa = sm_lds + tokl * 64 + (k & 1) * 8 + 4 * hh, gk = (unsigned)((k >> 1) ^ wa_g(tokl));
                LG::run(xv, j, k, 8 * k + 4 * hh, ln_fast, live, cC, cB, cSc, cY,
                       [&](int i, unsigned pk0, unsigned) __attribute__((always_inline)) {
                           *(lds_u32 *)(size_t)(rowa + (i >> 1) * G::KBLK + ((gk ^ ((i & 1) * 2)) << 4)) = pk0;
                       });
            }
        } else {
            // ---- the panel's tokens: global -> LDS by DMA, one token group of 16 per wave at a time
            for (int tg = wave; tg < n_own * 2; tg += 8) WA_DMA16(G::KB, G::KBLK, sm, 0, tg, lane, p.x, (long long)t0 * 32, p.M)
        }
        // output row offset of every token of the panel: (b * H * T + t_in_image) * 64
        if (tid < G::TOK) {
            const int row = min(t0 * 32 + tid, p.M - 1), b = row / p.T;
            reinterpret_cast<int *>(sm + G::SOFF)[tid] = (b * p.H * p.T + (row - b * p.T)) * 64;
            if constexpr (VT) reinterpret_cast<int *>(sm + G::SVOFF)[tid] = b * p.H * 64 * p.ldv + (row - b * p.T);
        }
        // tasks: (slab, token half); half a = tiles [0, na), half b = [na, n_own)
        const int na = (n_own + 1) >> 1, ntask = n_own > 1 ? 2 * ncp : ncp;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();

        const unsigned fa0 = sm_lds + tok * 64 + e * 16, fa1 = sm_lds + tok * 64 + (e ^ 2) * 16;
        for (int task = wave; task < ntask; task += 8) {
            const int half = task >= ncp, cp = task - half * ncp;
            const int tb0 = half ? na : 0, te = half ? n_own : na;
            // the slab's weights: NOT carried from task to task (loop-carried and redefined behind their last use, the compiler
            // copies all 96 registers at the back edge and spills); the partner wave of the SIMD works through the latency
            v4i W[2][G::KS];
            {
                const char *wq = reinterpret_cast<const char *>(p.wf + (size_t)cp * 2 * G::KS * 64);
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int ks = 0; ks < G::KS; ++ks) W[c][ks] = *reinterpret_cast<const v4i *>(wq + lane16 + (c * G::KS + ks) * 1024);
            }
            const int chb = 64 * cp + 16 * kh;
            const int which = EPI == WS_EPI_QKV8 ? cp / max(ncp3, 1) : 0;
            int8_t *obase = (which == 0 ? p.q : which == 1 ? p.k : p.v) + (size_t)(cp - which * ncp3) * p.T * 64 + 16 * kh;
            // v^T form: a V slab's lane (token, h) stores its 16 channels as 16 bytes, one per row of the head's [64][ldv] — the 32 lanes
            // of a half-wave are 32 consecutive tokens, so every store instruction writes runs of consecutive bytes (two where an image
            // boundary falls inside the tile).  Only tokens t < T exist, so the columns t >= T keep their zeros
            const bool vslab = VT && which == 2;
            int8_t *vbase = VT ? p.v + (size_t)((cp - 2 * ncp3) * 64 + 16 * kh) * p.ldv : nullptr;
            auto sweep = [&](auto nt_c, const int tb) __attribute__((always_inline)) {
                constexpr int NT = decltype(nt_c)::value;
                v4i bf[2][NT];
                v16i acc[2][NT];
                const unsigned fb0 = fa0 + tb * 2048, fb1 = fa1 + tb * 2048;
                int toff[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    toff[t] = *(lds_i32 *)(size_t)(sm_lds + (vslab ? G::SVOFF : G::SOFF) + ((tb + t) * 32 + tok) * 4);
                auto load_b = [&](int ks, int slot) __attribute__((always_inline)) {
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        bf[slot][t] = *(lds_v4i *)(size_t)(((ks & 1) ? fb1 : fb0) + (ks >> 1) * G::KBLK + t * 2048);
                };
                load_b(0, 0);
                // EPI_RES16: the identity rows of this sweep, requested in front of its K loop (a vector load issued behind the
                // previous sweep's stores would wait for them)
                v4i idr[EPI == WS_EPI_RES16 ? 2 : 1][EPI == WS_EPI_RES16 ? NT : 1][2];
                if constexpr (EPI == WS_EPI_RES16) {
#pragma unroll
                    for (int c = 0; c < 2; ++c)
#pragma unroll
                        for (int t = 0; t < NT; ++t) {
                            const long long row = min((long long)(t0 + tb + t) * 32 + tok, (long long)p.M - 1);
                            const int16_t *rp = p.residual + row * p.N + chb + 32 * c;
                            idr[c][t][0] = *reinterpret_cast<const v4i *>(rp);
                            idr[c][t][1] = *reinterpret_cast<const v4i *>(rp + 8);
                        }
                }
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    WA_ACC_BIAS(acc[c][0], *(lds_v4i *)(size_t)(sm_lds + G::SBIAS + (chb + 32 * c + 4 * q) * 4));
#pragma unroll
                    for (int t = 1; t < NT; ++t) acc[c][t] = acc[c][0];
                }
#pragma unroll
                for (int ks = 0; ks < G::KS; ++ks) {
                    __builtin_amdgcn_sched_barrier(0);
                    if (ks + 1 < G::KS) load_b(ks + 1, (ks + 1) & 1);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int c = 0; c < 2; ++c)
#pragma unroll
                        for (int t = 0; t < NT; ++t)
                            acc[c][t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(W[c][ks], bf[ks & 1][t], acc[c][t], 0, 0, 0);
                }
                // requant to 8 bits: fma(z, c, magic + 128) leaves Q + 128 in the low dword, wa_pack_biased clamps while packing,
                // the xor takes the bias off again.  One (channel tile, token tile) at a time:
                // sixteen channels of a token per lane, one 16-byte store
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    v2d cqv[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) cqv[j] = *(lds_v2d *)(size_t)(sm_lds + G::SCQ + (chb + 32 * c + 2 * j) * 8);
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        if constexpr (EPI == WS_EPI_RES16) {
                            // 16-bit requant, then the residual QuantAct
                            v4i o0, o1;
#pragma unroll
                            for (int d = 0; d < 8; ++d) {
                                const int pk = wa_res_pair<FMA>(acc[c][t][2 * d], acc[c][t][2 * d + 1], cqv[d], d < 4 ? idr[c][t][0][d] : idr[c][t][1][d - 4],
                                                                p.cm, p.cr, std::true_type{});
                                if (d < 4) o0[d] = pk; else o1[d - 4] = pk;
                            }
                            asm volatile("" : "+v"(o0), "+v"(o1));
                            const long long row = (long long)(t0 + tb + t) * 32 + tok;
                            if (row < p.M) {
                                int16_t *op = p.out16 + row * p.N + chb + 32 * c;
                                *reinterpret_cast<v4i *>(op) = o0;
                                *reinterpret_cast<v4i *>(op + 8) = o1;
                            }
                            continue;
                        }
                        v4i o4;
#pragma unroll
                        for (int q4 = 0; q4 < 4; ++q4) {
                            int o[4];
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const double m = cqv[2 * q4 + (i >> 1)][i & 1];
                                const double tq = FMA ? __builtin_fma((double)acc[c][t][4 * q4 + i], m, RQ_MAGIC + 128.0)
                                                      : ((double)acc[c][t][4 * q4 + i] * m + (RQ_MAGIC + 128.0));
                                o[i] = __double2loint(tq);
                            }
                            int hq = (int)(wa_pack_biased(o[0], o[1], o[2], o[3]) ^ 0x80808080u);
                            asm volatile("" : "+v"(hq));       // pinned: left alone, the optimiser converts every accumulator first
                            o4[q4] = hq;
                        }
                        const int row = (t0 + tb + t) * 32 + tok;
                        if constexpr (EPI == WS_EPI_RQ8) {
                            if (row < p.M) *reinterpret_cast<v4i *>(p.q + (long long)row * p.N + chb + 32 * c) = o4;
                        } else if (vslab) {
                            if (row < p.M) {
                                int8_t *vp = vbase + toff[t] + (size_t)(32 * c) * p.ldv;
#pragma unroll
                                for (int i = 0; i < 16; ++i) vp[(size_t)i * p.ldv] = (int8_t)(o4[i >> 2] >> (8 * (i & 3)));
                            }
                        } else if constexpr (G::MAXT > 8) {
                            // (the long-panel form predicates the store: with the select below the compiler keeps so much of the
                            // requant in flight across its sweep loop that the kernel spills)
                            if (row < p.M) *reinterpret_cast<v4i *>(obase + toff[t] + 32 * c) = o4;
                        } else {
                            *reinterpret_cast<v4i *>(row < p.M ? obase + toff[t] + 32 * c : (int8_t *)p.dummy + lane16) = o4;
                        }
                    }
                }
            };
            int tb = tb0;
            if constexpr (G::MAXT <= 8) {
                // a half has one to four tiles
                if (te - tb > 2) { sweep(std::integral_constant<int, 2>{}, tb); tb += 2; }
                if (te - tb == 2) sweep(std::integral_constant<int, 2>{}, tb);
                else sweep(std::integral_constant<int, 1>{}, tb);
            } else {
                // a half has one to MAXT / 2 tiles: pairs, then the odd one
                for (; te - tb >= 2; tb += 2) sweep(std::integral_constant<int, 2>{}, tb);
                if (te - tb == 1) sweep(std::integral_constant<int, 1>{}, tb);
            }
        }
        if constexpr (LN_TAIL) {
            // ---- norm2 + qact3 of the panel's rows (vit_quant.py:139-140): every channel of a row was produced by this workgroup;
            // its stores are complete (vmcnt) and no line of out16 was ever read through this CU's L1, so the rows come back from
            // the L2 they were just written to.  Same arithmetic as layernorm_reg_kernel<384, 2>, bytes to ln_out8 [M][384]
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            typedef LnGroup<G::K, 2> LG;
            const int j = lane & 7, k = j >> 1, hh = j & 1;
            const float ys = rcp_rn(p.ln_s);
            for (int r0 = wave * 8; r0 < n_own * 32; r0 += 64) {
                const long long row_raw = (long long)t0 * 32 + r0 + (lane >> 3);
                const bool live = row_raw < p.M;
                const long long row = live ? row_raw : (long long)p.M - 1;
                const int16_t *xp = p.out16 + row * G::K + 8 * k + 4 * hh;
                float xv[LG::NSTEP][LG::EPC];
                LN_ROW_X(LG, xv, LG::raw_at(xp + 32 * i), p.ln_s, ys);
                LG::run(xv, j, k, 8 * k + 4 * hh, ln_fast, live, cC, cB, cSc, cY, p.ln_out8 + row * G::K + 8 * k + 4 * hh);
            }
        }
    }
}
