// ivit_mlp192.h — Mlp.forward + the block's residual QuantAct as ONE kernel at width 192 (DeiT-Tiny: every block; Swin-T / S: stage 1):
//   fc1 -> qact_gelu (8 bit) -> ShiftGELU -> qact1 (8 bit) -> fc2 -> qact2 (16 bit) -> qact4(+identity) (16 bit)
// (models/layers_quant.py:144-153, then vit_quant.py:141-142 / swin_quant.py:296-300).  The scheme of ivit_mlp.h (weights in
// MFMA-fragment order streamed L2 -> registers, the hidden tile of a unit in LDS only, no barrier inside the GEMM phases)
// re-cut for a 768-byte hidden row:
//
//   * a unit is up to 80 tokens: hidden 80 x 768 B = 60 KB + activations 80 x 192 B = 15 KB + table lines 2 KB = 77 KB of
//     LDS, so TWO workgroups of four waves share a CU (154 KB of 160) and one of them multiplies while the other is in its
//     ShiftGELU phase or waits at a barrier;
//   * one pass over both weight matrices is 288 KB (1.18 MB at width 384), i.e. 3.7 KB per token of a full unit against
//     14.7 KB there;
//   * fc2's 12 output-channel tiles split as 4 waves x 3 tiles, fc1's 48 as 4 waves x 4 chunks of 3: the register picture
//     of a wave (3 channel tiles x 5 token tiles of accumulators) is the one mlp384_kernel has at eight waves.
//
// Shapes: v_mfma_i32_16x16x64_i8, weights as the A operand (rows = channels), activations as B (columns = tokens): a lane
// holds 4 consecutive channels of one token per accumulator, which pack into one dword.  LDS images are K-blocked,
// [64-column block][80 tokens][64 B], with the chunk permutation mlp_phi of ivit_mlp.h (conflict-free ds_read_b128).
#pragma once
#include <type_traits>
#include "ivit_device.h"
#include "ivit_mlp.h"

#define M192_C 192
#define M192_HD 768
#define M192_TT 5                                 // token tiles (of 16) a unit may have: 4 or 5
#define M192_WAVES 4
#define M192_NJ 3                                 // channel tiles per wave and step
#define M192_THREADS (M192_WAVES * 64)
#define M192_KS1 (M192_C / 64)                    // 3 column steps of fc1
#define M192_KS2 (M192_HD / 64)                   // 12 column steps of fc2
#define M192_KBLK (M192_TT * 16 * 64)             // one 64-column block of an LDS image: [80 tokens][64 B]
#define M192_SH 0                                 // hidden tile [12][80][64 B]
#define M192_SA (M192_KS2 * M192_KBLK)            // activation tile [3][80][64 B]
#define M192_STAB (M192_SA + M192_KS1 * M192_KBLK)    // one ShiftGELU table line (256 B) per half-wave
#define M192_SMEM (M192_STAB + 2 * M192_WAVES * 256)
#define M192_WG_PER_CU 2
#define M192_WD 3                                 // weight fragments in flight ahead of the MFMAs that consume them

struct Mlp192Args {
    const int8_t *x;          // [M, 192] int8 (LayerNorm + requant output)
    const v4i *w1f, *w2f;     // fragment-ordered weights (mlp192_swizzle_kernel)
    const int32_t *b1, *b2;   // biases (never null: the plans' bias_eff)
    const double *cq1, *cq2;  // per-channel c = m * 2^-e
    const int8_t *tab;        // ShiftGELU(+requant) table [256 maxima][256 values]
    const int16_t *residual;  // [M, 192] identity branch
    int16_t *out;             // [M, 192]
    double cm, cr;            // qact4: main and identity multipliers
    long long M;
};

// weights [N][K] int8 -> fragments of 64 lanes x 16 B, lane l = W[ct*16 + (l & 15)][ks*64 + (l >> 4)*16 ...], in the order the
// kernel consumes them: fragment f = step * 12 + wave * 3 + j, step = chunk * (K / 64) + ks, channel tile
// ct = wave * T + chunk * 3 + j with T = N / 16 / 4 tiles per wave.  What the four waves request in one step is one
// contiguous 12 KB window.
__global__ __launch_bounds__(256) void mlp192_swizzle_kernel(const int8_t *__restrict__ w, int N, int K, v4i *__restrict__ wf) {
    const int nks = K >> 6, T = (N >> 4) / M192_WAVES;
    const long long total = (long long)(N >> 4) * nks * 64;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int l = (int)(i & 63);
        const int f = (int)(i >> 6), step = f / (M192_NJ * M192_WAVES), r = f - step * (M192_NJ * M192_WAVES);
        const int chunk = step / nks, ks = step - chunk * nks, ct = (r / M192_NJ) * T + chunk * M192_NJ + (r % M192_NJ);
        wf[i] = *reinterpret_cast<const v4i *>(w + (long long)(ct * 16 + (l & 15)) * K + ks * 64 + (l >> 4) * 16);
    }
}

// FMA: both plans prove |z * m| < 2^53 (one fused rounding == the reference's two), else multiply and add separately.
// Both plans prove |z * c| < 2^31 (the host refuses the kernel otherwise); |cm|, |cr| < 2^9 (host-checked) for rq_fast.
//
// Units: the token axis is cut into tiles of 16; workgroup b owns the contiguous tile range [T b / G, T (b + 1) / G) and walks
// it in equal units of <= 5 tiles (a unit costs one pass over both weight matrices whatever its size, so units are as large
// as the LDS allows and as few as possible).  The unit body is instantiated for 4 and for 5 tiles; a unit with fewer tiles
// runs the 4-tile body on clamped rows and stores only its own.
//
// Software pipeline of both GEMM phases as in mlp384_kernel: step s issues the weight fragments of step s + WD and the
// activation fragments of step s + 1, then its own MFMAs (pinned with scheduling fences).
template <bool FMA>
__global__ __launch_bounds__(M192_THREADS, 2) void mlp192_kernel(Mlp192Args p) {
    extern __shared__ __attribute__((aligned(256))) char sm[];
    constexpr int NJ = M192_NJ;
    constexpr int CT1 = M192_HD / 16 / M192_WAVES;    // 12 channel tiles of fc1 per wave, in chunks of NJ
    constexpr int NCH = CT1 / NJ, NS1 = NCH * M192_KS1, WD = M192_WD;   // fc1 chunks, fc1 steps, weight prefetch distance
    constexpr int ACH = M192_C / 16;                  // 16-byte chunks of an activation row
    constexpr int AREG = (M192_TT * 16 * ACH + M192_THREADS - 1) / M192_THREADS;
    static_assert(NJ * 16 * M192_WAVES == M192_C && CT1 % NJ == 0, "wave count must split 48 / 12 channel tiles evenly");
    static_assert(M192_KS1 >= 3, "the fc1 pipeline loads a chunk's multipliers at its first step and the next bias at its second");
    static_assert(M192_WG_PER_CU * M192_SMEM <= 160 * 1024, "two workgroups per CU");
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    typedef double v2d __attribute__((ext_vector_type(2)));

    // ---- this workgroup's units: (first tile, tiles) of unit i
    const long long ntiles = (p.M + 15) >> 4;
    const long long t_beg = ntiles * blockIdx.x / gridDim.x, t_end = ntiles * (blockIdx.x + 1) / gridDim.x;
    const int n_own = (int)(t_end - t_beg);
    const int nu = (n_own + M192_TT - 1) / M192_TT;
    if (nu <= 0) return;
    auto unit_tile0 = [&](int i) -> long long { return t_beg + (long long)n_own * i / nu; };
    auto unit_ntt = [&](int i) -> int { return i >= nu ? 0 : (int)(unit_tile0(i + 1) - unit_tile0(i)); };

    // activation tile of a unit (rows x 12 chunks of 16 B): global -> registers (a_fetch), registers -> LDS (a_commit).  Row and
    // chunk of a lane come from an opaque copy of the thread id: left visible, the eight per-lane addresses are hoisted out of
    // the unit loop and spilled
    v4i areg[AREG];
    auto a_fetch = [&](long long tile0, int ntt) __attribute__((always_inline)) {
        int t = threadIdx.x;
        asm volatile("" : "+v"(t));
#pragma unroll
        for (int i = 0; i < AREG; ++i) {
            const int ch = t + i * M192_THREADS, row = ch / ACH, c16 = ch - row * ACH;
            if (ch < ntt * 16 * ACH) {
                const long long grow = min(tile0 * 16 + row, p.M - 1);
                areg[i] = *reinterpret_cast<const v4i *>(p.x + grow * M192_C + c16 * 16);
            }
        }
    };
    auto a_commit = [&](int ntt) __attribute__((always_inline)) {
        int t = threadIdx.x;
        asm volatile("" : "+v"(t));
#pragma unroll
        for (int i = 0; i < AREG; ++i) {
            const int ch = t + i * M192_THREADS, row = ch / ACH, c16 = ch - row * ACH;
            if (ch < ntt * 16 * ACH)
                *reinterpret_cast<v4i *>(sm + M192_SA + (c16 >> 2) * M192_KBLK + row * 64 + mlp_phi(row, c16 & 3) * 16) = areg[i];
        }
    };

    // ------------------------------------------------------------------------------------------------------------------
    // one unit of NTT token tiles starting at tile `tile0`; (next_tile0, next_ntt): the unit whose activations to prefetch
    // Barriers: B1 before the first hidden write (every wave is done reading the previous unit's hidden tile; placed AFTER the
    // first chunk's K loop), B2 hidden tile complete / activation tile dead, B3 hidden tile rewritten by ShiftGELU and the
    // NEXT unit's activation tile committed.
    auto unit_body = [&](auto ntt_c, const int ntt, const long long tile0, const long long next_tile0, const int next_ntt) __attribute__((always_inline)) {
        constexpr int NTT = decltype(ntt_c)::value;       // tiles the body multiplies; `ntt` <= NTT of them belong to this unit
        const long long tok0 = tile0 * 16;
        // per-lane indices from an opaque copy of the thread id (keeps the unrolled phases' LDS addresses from being hoisted
        // out of the unit loop into registers)
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63, tl = lane & 15, g = lane >> 4;
        const unsigned fb = tl * 64 + mlp_phi(tl, g) * 16;          // this lane's B-fragment chunk inside a K block, token tile 0

        // ---- fc1 + qact_gelu (8 bit) into the hidden tile
        {
            const v4i *w1 = p.w1f + (size_t)(wave * NJ) * 64 + lane;
            v4i wf[WD + 1][NJ], bf[2][NTT], acc[NJ][NTT], bias_n[NJ];
            v2d cq[NJ][2];
            auto load_w = [&](int s, int slot) __attribute__((always_inline)) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) wf[slot][j] = w1[(size_t)(s * NJ * M192_WAVES + j) * 64];
            };
            auto load_b = [&](int s, int slot) __attribute__((always_inline)) {
                const int ks = s % M192_KS1;
#pragma unroll
                for (int tt = 0; tt < NTT; ++tt)
                    bf[slot][tt] = *reinterpret_cast<const v4i *>(sm + M192_SA + ks * M192_KBLK + tt * 1024 + fb);
            };
            auto load_bias = [&](int chunk) __attribute__((always_inline)) {
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                    bias_n[j] = *reinterpret_cast<const v4i *>(p.b1 + (wave * CT1 + chunk * NJ + j) * 16 + 4 * g);
            };
#pragma unroll
            for (int s = 0; s < WD; ++s) load_w(s, s);
            load_b(0, 0);
            load_bias(0);
#pragma unroll
            for (int s = 0; s < NS1; ++s) {
                const int chunk = s / M192_KS1, ks = s - chunk * M192_KS1, ct0 = wave * CT1 + chunk * NJ;
                __builtin_amdgcn_sched_barrier(0);
                if (s + WD < NS1) load_w(s + WD, (s + WD) % (WD + 1));
                if (s + 1 < NS1) load_b(s + 1, (s + 1) & 1);
                if (ks == 0) {                       // this chunk's multipliers: consumed two steps on
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        const int ch0 = (ct0 + j) * 16 + 4 * g;
                        cq[j][0] = *reinterpret_cast<const v2d *>(p.cq1 + ch0);
                        cq[j][1] = *reinterpret_cast<const v2d *>(p.cq1 + ch0 + 2);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                if (ks == 0) {
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
#pragma unroll
                        for (int tt = 0; tt < NTT; ++tt) acc[j][tt] = bias_n[j];
                }
                if (ks == 1 && chunk + 1 < NCH) load_bias(chunk + 1);      // the next chunk's bias, two steps ahead
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int tt = 0; tt < NTT; ++tt)
                        acc[j][tt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf[s % (WD + 1)][j], bf[s & 1][tt], acc[j][tt], 0, 0, 0);
                if (ks == M192_KS1 - 1) {
                    if (chunk == 0) __syncthreads();                       // B1: the hidden tile is free
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        const int ch0 = (ct0 + j) * 16 + 4 * g;               // this lane's 4 hidden channels
                        const int kb = ch0 >> 6, cc = (ch0 >> 4) & 3;           // fc2 K block and chunk of these channels
#pragma unroll
                        for (int tt = 0; tt < NTT; ++tt) {
                            int o[4];
                            o[0] = mlp_rq<FMA>(acc[j][tt][0], cq[j][0][0]);
                            o[1] = mlp_rq<FMA>(acc[j][tt][1], cq[j][0][1]);
                            o[2] = mlp_rq<FMA>(acc[j][tt][2], cq[j][1][0]);
                            o[3] = mlp_rq<FMA>(acc[j][tt][3], cq[j][1][1]);
#pragma unroll
                            for (int e = 0; e < 4; ++e) o[e] = min(max(o[e], -128), 127);
                            const unsigned w01 = __builtin_amdgcn_perm((unsigned)o[1], (unsigned)o[0], 0x0c0c0400u);
                            const unsigned w23 = __builtin_amdgcn_perm((unsigned)o[3], (unsigned)o[2], 0x0c0c0400u);
                            const int tok = tt * 16 + tl;
                            *reinterpret_cast<unsigned *>(sm + M192_SH + kb * M192_KBLK + tok * 64 + mlp_phi(tok, cc) * 16 + 4 * g) =
                                __builtin_amdgcn_perm(w23, w01, 0x05040100u);
                        }
                    }
                }
            }
        }
        __syncthreads();                                                    // B2

        // ---- ShiftGELU (+ qact1) in place, half a wavefront per token, NTT * 2 tokens per half-wave: the token's 768 hidden
        // bytes are read once (6 dwords per lane) and stay in registers from the row maximum (packed byte maxima, then 5
        // shuffles) over the fetch of the maximum's 256-byte table line (global -> this half-wave's LDS slot) to the byte
        // gathers and the write-back.  No workgroup barrier inside.  The next unit's activations travel meanwhile.
        if (next_ntt > 0) a_fetch(next_tile0, next_ntt);
        {
            const int hw = wave * 2 + (lane >> 5), l32 = lane & 31;
            typedef __attribute__((address_space(3))) const unsigned char lds_u8;
            typedef unsigned short v2us __attribute__((ext_vector_type(2)));
            const unsigned sm_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char *)sm;
            const unsigned base = sm_lds + M192_STAB + hw * 256;           // 256-byte aligned: byte | base is the address
            constexpr int NW = M192_KS2 / 2;                                 // dwords of a row per lane
            constexpr int NTOK = (NTT * 16 + 2 * M192_WAVES - 1) / (2 * M192_WAVES);     // tokens per half-wave
            unsigned w[NTOK][NW];
            v2i line[NTOK];
            // pass 1: rows -> registers, row maxima, all table-line requests in flight together
#pragma unroll
            for (int i = 0; i < NTOK; ++i) {
                const int t = hw + i * 2 * M192_WAVES;
                if (t < NTT * 16) {
                    const unsigned *hp = reinterpret_cast<const unsigned *>(sm + M192_SH + t * 64) + (l32 & 15) + (l32 >> 4) * (M192_KBLK / 4);
                    v2us me = {0, 0}, mo = {0, 0};                          // running maxima of the even / odd bytes (biased)
#pragma unroll
                    for (int m = 0; m < NW; ++m) {
                        w[i][m] = hp[m * (M192_KBLK / 2)] ^ 0x80808080u;    // K blocks 2m, 2m + 1 (the upper 16 lanes): Q + 128
                        me = __builtin_elementwise_max(me, __builtin_bit_cast(v2us, __builtin_amdgcn_perm(0u, w[i][m], 0x0c020c00u)));
                        mo = __builtin_elementwise_max(mo, __builtin_bit_cast(v2us, __builtin_amdgcn_perm(0u, w[i][m], 0x0c030c01u)));
                    }
                    const v2us m2 = __builtin_elementwise_max(me, mo);
                    int qb = max((int)m2[0], (int)m2[1]);                    // biased row maximum of this lane
#pragma unroll
                    for (int o = 16; o > 0; o >>= 1) qb = max(qb, __shfl_xor(qb, o));
                    line[i] = reinterpret_cast<const v2i *>(p.tab + (size_t)qb * 256)[l32];
                }
            }
            // pass 2: table line -> this half-wave's LDS slot, byte gathers, write-back.  Wave-level ordering only: the slot
            // belongs to this half-wave and the previous token's gathers were consumed by its write-back
#pragma unroll
            for (int i = 0; i < NTOK; ++i) {
                const int t = hw + i * 2 * M192_WAVES;
                if (t < NTT * 16) {
                    unsigned *hp = reinterpret_cast<unsigned *>(sm + M192_SH + t * 64) + (l32 & 15) + (l32 >> 4) * (M192_KBLK / 4);
                    reinterpret_cast<v2i *>(sm + M192_STAB + hw * 256)[l32] = line[i];
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
                    for (int m = 0; m < NW; ++m) {
                        const unsigned x = w[i][m];
                        const unsigned b0 = *(lds_u8 *)(size_t)(base | (x & 0xffu)), b1 = *(lds_u8 *)(size_t)(base | ((x >> 8) & 0xffu));
                        const unsigned b2 = *(lds_u8 *)(size_t)(base | ((x >> 16) & 0xffu)), b3 = *(lds_u8 *)(size_t)(base | (x >> 24));
                        hp[m * (M192_KBLK / 2)] = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
                    }
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                }
            }
        }
        if (next_ntt > 0) a_commit(next_ntt);
        __syncthreads();                                                    // B3

        // ---- fc2 + qact2 (16 bit) + qact4 with the identity branch (16 bit)
        {
            const v4i *w2 = p.w2f + (size_t)(wave * NJ) * 64 + lane;
            v4i wf[WD + 1][NJ], bf[2][NTT], acc[NJ][NTT];
            auto load_w = [&](int s, int slot) __attribute__((always_inline)) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) wf[slot][j] = w2[(size_t)(s * NJ * M192_WAVES + j) * 64];
            };
            auto load_b = [&](int s, int slot) __attribute__((always_inline)) {
#pragma unroll
                for (int tt = 0; tt < NTT; ++tt)
                    bf[slot][tt] = *reinterpret_cast<const v4i *>(sm + M192_SH + s * M192_KBLK + tt * 1024 + fb);
            };
#pragma unroll
            for (int s = 0; s < WD; ++s) load_w(s, s);
            load_b(0, 0);
            // identity rows and multipliers of this lane's outputs: requested now, consumed after the K loop
            v2i rs[NJ][NTT];
            v2d c2[NJ][2];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int ch0 = (wave * NJ + j) * 16 + 4 * g;
                c2[j][0] = *reinterpret_cast<const v2d *>(p.cq2 + ch0);
                c2[j][1] = *reinterpret_cast<const v2d *>(p.cq2 + ch0 + 2);
                const v4i b4 = *reinterpret_cast<const v4i *>(p.b2 + ch0);
#pragma unroll
                for (int tt = 0; tt < NTT; ++tt) {
                    acc[j][tt] = b4;
                    const long long tok = min(tok0 + tt * 16 + tl, p.M - 1);
                    rs[j][tt] = *reinterpret_cast<const v2i *>(p.residual + tok * M192_C + ch0);
                }
            }
#pragma unroll
            for (int s = 0; s < M192_KS2; ++s) {
                __builtin_amdgcn_sched_barrier(0);
                if (s + WD < M192_KS2) load_w(s + WD, (s + WD) % (WD + 1));
                if (s + 1 < M192_KS2) load_b(s + 1, (s + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int tt = 0; tt < NTT; ++tt)
                        acc[j][tt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf[s % (WD + 1)][j], bf[s & 1][tt], acc[j][tt], 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int ch0 = (wave * NJ + j) * 16 + 4 * g;
#pragma unroll
                for (int tt = 0; tt < NTT; ++tt) {
                    int t16[4];
                    t16[0] = mlp_rq<FMA>(acc[j][tt][0], c2[j][0][0]);
                    t16[1] = mlp_rq<FMA>(acc[j][tt][1], c2[j][0][1]);
                    t16[2] = mlp_rq<FMA>(acc[j][tt][2], c2[j][1][0]);
                    t16[3] = mlp_rq<FMA>(acc[j][tt][3], c2[j][1][1]);
                    int o[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int t = min(max(t16[e], -32768), 32767);
                        const int r = (int)(short)((unsigned)rs[j][tt][e >> 1] >> (16 * (e & 1)));
                        // both terms are integers < 2^31: the sum is the reference's fp64 sum (quant_utils.py:238-244)
                        o[e] = min(max(rq_fast(r, p.cr) + rq_fast(t, p.cm), -32768), 32767);
                    }
                    const long long tok = tok0 + tt * 16 + tl;
                    if (tok < p.M && tt < ntt)         // a short unit's surplus tiles belong to the next unit
                        *reinterpret_cast<v2i *>(p.out + tok * M192_C + ch0) =
                            v2i{(int)__builtin_amdgcn_perm((unsigned)o[1], (unsigned)o[0], 0x05040100u),
                                (int)__builtin_amdgcn_perm((unsigned)o[3], (unsigned)o[2], 0x05040100u)};
                }
            }
        }
    };

    // ---- the unit stream
    a_fetch(unit_tile0(0), unit_ntt(0));
    a_commit(unit_ntt(0));
    __syncthreads();
    for (int i = 0; i < nu; ++i) {
        const long long tile0 = unit_tile0(i), tile1 = unit_tile0(i + 1);
        const int ntt = unit_ntt(i), next_ntt = unit_ntt(i + 1);
        if (ntt == M192_TT) unit_body(std::integral_constant<int, M192_TT>{}, ntt, tile0, tile1, next_ntt);
        else unit_body(std::integral_constant<int, M192_TT - 1>{}, ntt, tile0, tile1, next_ntt);
    }
}
