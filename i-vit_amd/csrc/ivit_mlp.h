// ivit_mlp.h — Mlp.forward + the block's residual QuantAct as ONE kernel for the D = 384 models (DeiT-S, Swin stage 2) and, with
// the same body re-cut (below: "Width 192", "Width 256", "Width 128"), the D = 192 ones (DeiT-Tiny: every block; Swin-T / S: stage 1)
// and Swin-B's stages 1 and 0:
//   fc1 -> qact_gelu (8 bit) -> ShiftGELU -> qact1 (8 bit) -> fc2 -> qact2 (16 bit) -> qact4(+identity) (16 bit)
// (models/layers_quant.py:144-153, then vit_quant.py:141-142 / swin_quant.py:296-300).  The 4 D-wide hidden tensor never
// exists in HBM: per 64-token unit it is produced into LDS by fc1, rewritten in place by the ShiftGELU table and consumed
// from LDS by fc2.  Unfused, the hidden tensor crosses HBM four times (fc1 write, GELU read + write, fc2 read: 310 MB of
// the layer's 775 MB at batch 256) and ShiftGELU is a launch of its own.
//
// Why 64 tokens and why it pays although each unit re-reads both weight matrices (1.18 MB) from L2: ShiftGELU's row
// maximum couples all 1536 hidden channels of a token, so a unit must own whole hidden rows; 64 rows x 1536 B = 96 KB is
// what the LDS holds next to the activation tile.  The weights stream L2 -> registers (never through LDS): they are laid
// out at plan time in MFMA-fragment order (1 KB per (16-channel tile, 64-column step), lane-linear), every wave reads only
// the fragments of ITS output channels, and a fragment feeds four MFMAs (four 16-token tiles).  No barrier inside the two
// GEMM phases: the eight waves drift apart, one wave's requant epilogue runs beside its SIMD mate's MFMAs.
//
// Shapes: v_mfma_i32_16x16x64_i8, weights as the A operand (rows = channels), activations as B (columns = tokens): a lane
// holds 4 consecutive channels of one token per accumulator, which pack into one dword.  fc1: wave w owns hidden channels
// [192 w, 192 w + 192) in four chunks of 48 (3 channel tiles x 4 token tiles = 48 accumulator registers); fc2: wave w owns
// output channels [48 w, 48 w + 48).  288 MFMAs per wave and phase.
//
// LDS images are K-blocked, [64-column block][64 tokens][64 B], with the four 16-byte chunks of a token's 64 B permuted by
// phi(token, chunk) = swapbits(chunk) ^ ((token >> 3) & 1): a ds_read_b128 is served in four groups of 16 lanes whose
// (token, chunk) sets are {0-3, 12-15} x {c} with {4-11} x {c + 1} (and the mirror image) — a row-major image with any
// padded stride has a 2-way conflict in every group; this permutation has none and needs no padding.
//
// Width 192 (mlp192_kernel; hidden row 768 B).  A unit of up to 80 tokens is hidden 60 KB + activations 15 KB + table lines 2 KB =
// 77 KB of LDS, so TWO workgroups of four waves share a CU (154 KB of 160): one of them multiplies while the other is in its
// ShiftGELU phase or waits at a barrier.  One pass over both weight matrices is 288 KB (1.18 MB at width 384), i.e. 3.7 KB per
// token of a full unit against 14.7 KB there.  fc2's 12 output-channel tiles split as 4 waves x 3 tiles, fc1's 48 as 4 waves x 4
// chunks of 3: the register picture of a wave (3 channel tiles x 5 token tiles of accumulators) is the one mlp384_kernel has at
// eight waves.  Units are always contiguous tile ranges.  The LayerNorm-headed form is mlp192ln_kernel (below): norm2's constants
// take the 3 KB that two workgroups leave of the CU's LDS.
//
// Width 256 (mlp256_kernel; Swin-B stage 1, hidden row 1024 B).  Eight waves, two channel tiles each (NJ = 2): fc1's 64 tiles are
// 8 waves x 4 chunks of 2, fc2's 16 are 8 x 2.  Hidden 80 KB + activations 20 KB + table lines 4 KB = 104 KB: one workgroup per
// CU.  One pass over both weight matrices is 512 KB, 6.6 KB per token of a full unit.  Contiguous tile ranges, lock-step only.
//
// Width 128 (mlp128_kernel; Swin-B stage 0, hidden row 512 B), behind the STATELESS entry ivit_mlp_fused: there is no plan, so
// nothing is laid out or precomputed for it (G::DIRECT).  The weights are read row-major — a fragment of the lock-step layout
// is 16 rows x 64 contiguous bytes of W, so a lane loads its 16 bytes from W[(ct * 16 + (l & 15)) * K + ks * 64 + (l >> 4) * 16];
// both matrices are 128 KB and stay in L2 — the multipliers are m * 2^-e of the caller's ivit_dyadic tables, formed where
// they are consumed, a null bias is zeros, and the requant form is chosen at run time, once per workgroup: the magic-number
// form where |z c| < 2^31 holds for every channel, v_rndne_f64 + saturating convert otherwise (as swin_mlp_rs_kernel does at
// C = 96, whose whole-launch register-resident weights would be 128 KB over 16 waves here and do not fit).  Four waves, NJ = 2;
// hidden 40 KB + activations 10 KB + table lines 2 KB = 52 KB.  TWO workgroups share a CU (199 VGPRs, no scratch).  Three fit the
// LDS (156 of 160 KB) but not the registers: at <= 168 VGPRs the unit body keeps 128 B per lane in scratch (20 B with units of 4
// tiles and a prefetch distance of 2), and measured on one box against this cut it wins only at one unit per workgroup
// (50 176 tokens: 37 against 43 us) and loses at 12 544 (31 against 22 us, the chain: 27) and at 200 704 (122 against 114-120):
// profiles/README.md.  fc1 has two column steps per chunk: a chunk's multipliers and the next chunk's bias are both requested at
// step 0.
#pragma once
#include <type_traits>
#include "ivit_device.h"
#include "ivit_layernorm.h"

// The geometry of the lock-step kernel: everything follows from the width C and the wave count, except the five constants each
// width states itself (below).
template <int C_, int WAVES_>
struct MlpGeo {
    static constexpr int C = C_, HD = 4 * C_;
    static constexpr int TT = 5;                            // token tiles (of 16) a unit may have: 4 or 5
    static constexpr int WAVES = WAVES_;
    static constexpr int NJ = C / 16 / WAVES;               // channel tiles per wave and step: 3 at widths 384 and 192 (2 with 12 waves), 2 at 256 and 128
    //                         // waves / 4 per SIMD: a lone wave issues a 16x16x64 MFMA every ~34 cycles, the pipe takes one per ~17
    static constexpr int THREADS = WAVES * 64;
    static constexpr int KS1 = C / 64, KS2 = HD / 64;       // column steps of fc1 (6 / 4 / 3 / 2) and of fc2 (24 / 16 / 12 / 8)
    static constexpr int KBLK = TT * 16 * 64;               // one 64-column block of an LDS image: [80 tokens][64 B]
    static constexpr int SH = 0;                            // hidden tile [KS2][80][64 B]
    static constexpr int SA = KS2 * KBLK;                   // activation tile [KS1][80][64 B]
    static constexpr int STAB = SA + KS1 * KBLK;            // one ShiftGELU table line (256 B) per half-wave
    static constexpr int SMEM = STAB + 2 * WAVES * 256;
    static constexpr int SLN = SMEM;                        // LayerNorm-headed form: norm2's constants, 16 B per channel (c fp64, bias_int, sc)
    static constexpr int SMEM_LN = SLN + 16 * C;            // 80 KB x 2 at width 192, 160 KB x 1 at 384: exactly a CU's LDS
    static constexpr int WD = 3;                            // weight fragments in flight ahead of the MFMAs that consume them
    static constexpr bool DIRECT = false;                   // operands as a plan prepared them (fragment-ordered weights, c = m * 2^-e, a bias)
};
struct Mlp384Geo : MlpGeo<384, 8> {
    static constexpr int WG_PER_CU = 1;                     // 154 KB of LDS
    static constexpr int CQ_STEP = 1, BIAS_STEP = 2;        // fc1 step of a chunk that loads its multipliers / the next chunk's bias
    static constexpr bool OPAQUE_A = false;                 // a_fetch / a_commit index from the plain thread id
    static constexpr bool ROUND_ROBIN = true;               // MlpArgs::balanced picks between the two unit schedules
};
struct Mlp192Geo : MlpGeo<192, 4> {
    static constexpr int WG_PER_CU = 2;                     // 2 x 77 KB of LDS
    static constexpr int CQ_STEP = 0, BIAS_STEP = 1;        // fc1 has only 3 column steps: both loads one step earlier
    static constexpr bool OPAQUE_A = true;                  // left visible, the eight per-lane addresses of a_fetch / a_commit are
    //                                                         hoisted out of the unit loop and spilled
    static constexpr bool ROUND_ROBIN = false;              // contiguous tile ranges only: the round-robin branch compiles away
};
struct Mlp256Geo : MlpGeo<256, 8> {
    static constexpr int WG_PER_CU = 1;                     // 104 KB of LDS
    static constexpr int CQ_STEP = 1, BIAS_STEP = 2;        // fc1 has 4 column steps
    static constexpr bool OPAQUE_A = false;
    static constexpr bool ROUND_ROBIN = false;
};
struct Mlp128Geo : MlpGeo<128, 4> {
    static constexpr int WG_PER_CU = 2;                     // 2 x 52 KB of LDS; a third does not fit the registers (above)
    static constexpr int CQ_STEP = 0, BIAS_STEP = 0;        // fc1 has only 2 column steps: both loads at the first
    static constexpr bool OPAQUE_A = true;
    static constexpr bool ROUND_ROBIN = false;
    static constexpr bool DIRECT = true;                    // ivit_mlp_fused's operands as the caller holds them: row-major int8 weights, ivit_dyadic
    //                                                         tables, biases that may be null (MlpArgs: the same fields, re-read)
};
// width 384 by its old names (ivit_mlp_rs.h, the host side, tools/ubench/mlpr_experiment)
#define MLP_C Mlp384Geo::C
#define MLP_HD Mlp384Geo::HD
#define MLP_TT Mlp384Geo::TT
#define MLP_THREADS Mlp384Geo::THREADS
#define MLP_KS1 Mlp384Geo::KS1
#define MLP_KS2 Mlp384Geo::KS2
#define MLP_SMEM Mlp384Geo::SMEM

struct MlpArgs {
    const int8_t *x;          // [M, C] int8 (LayerNorm + requant output)
    const v4i *w1f, *w2f;     // fragment-ordered weights (mlp_swizzle_kernel / mlp256_swizzle_kernel / mlp192_swizzle_kernel)
    const int32_t *b1, *b2;   // biases (never null: the plans' bias_eff)
    const double *cq1, *cq2;  // per-channel c = m * 2^-e
    const int8_t *tab;        // ShiftGELU(+requant) table [256 maxima][256 values]
    const int16_t *residual;  // [M, C] identity branch
    int16_t *out;             // [M, C]
    double cm, cr;            // qact4: main and identity multipliers
    long long M;
    // G::DIRECT (mlp128_kernel): w1f / w2f are the row-major int8 matrices [HD][C] / [C][HD], cq1 / cq2 the ivit_dyadic tables
    // (m, 2^-e) of the two layers, b1 / b2 may be null
    // width 384 only from here on (the other widths read none of it)
    int balanced;             // unit schedule: 0 = 64-token units dealt round-robin, 1 = contiguous tile ranges cut into units of <= 5 tiles
    // mlp384rs_kernel<FMA, LNH = true> (ivit_layernorm_mlp_fused_planned): norm2 + qact3 of this workgroup's rows first, from the block's 16-bit
    // stream (`residual` is that stream), into x (a scratch of M x 384 bytes that only this launch reads)
    // mlp384ln_kernel / mlp192ln_kernel (ivit_layernorm_mlp_lockstep_planned), at both widths: the same operands, x unused — norm2's
    // rows go straight into the unit's activation tile
    float ln_s;
    const float *ln_bias_int, *ln_sc;
    const ivit_dyadic *ln_dy;
};

__device__ __forceinline__ int mlp_phi(int tok, int chunk) {
    return (((chunk & 1) << 1) | (chunk >> 1)) ^ ((tok >> 3) & 1);
}

// weights [N][K] int8 -> fragments of 64 lanes x 16 B, lane l = W[ct*16 + (l & 15)][ks*64 + (l >> 4)*16 ...], in the order the
// kernel consumes them: fragment index f = step * NJ * WAVES + wave * NJ + j, where step = chunk * (K / 64) + ks walks the wave's
// chunks of NJ channel tiles (ct = wave * T + chunk * NJ + j, T = N / 16 / WAVES tiles per wave) and the 64-column steps inside
// a chunk.  What the waves of a workgroup request in one step is ONE contiguous window (24 KB at width 384, 12 KB at 192): the
// requests spread over all L2 channels.  (With each wave's fragments contiguous instead — 24 streams a multiple of 4 KB
// apart advancing in lock-step — the fc2 weight stream ran at half the rate of the fc1 one: +9.5k cycles per unit.)
// One body under both kernel names.  A macro: called as an inlined helper the same loop compiles with two operands of one add
// swapped, and this form is proven to give the instruction streams the two hand-written copies had.
#define MLP_SWIZZLE_KERNEL(NAME, G)                                                                                     \
    __global__ __launch_bounds__(256) void NAME(const int8_t *__restrict__ w, int N, int K, v4i *__restrict__ wf) {     \
        const int nks = K >> 6, T = (N >> 4) / G::WAVES;                                                                \
        const long long total = (long long)(N >> 4) * nks * 64;                                                         \
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {     \
            const int l = (int)(i & 63);                                                                                \
            const int f = (int)(i >> 6), step = f / (G::NJ * G::WAVES), r = f - step * (G::NJ * G::WAVES);              \
            const int chunk = step / nks, ks = step - chunk * nks, ct = (r / G::NJ) * T + chunk * G::NJ + (r % G::NJ);  \
            wf[i] = *reinterpret_cast<const v4i *>(w + (long long)(ct * 16 + (l & 15)) * K + ks * 64 + (l >> 4) * 16);  \
        }                                                                                                               \
    }
MLP_SWIZZLE_KERNEL(mlp_swizzle_kernel, Mlp384Geo)
MLP_SWIZZLE_KERNEL(mlp192_swizzle_kernel, Mlp192Geo)
MLP_SWIZZLE_KERNEL(mlp256_swizzle_kernel, Mlp256Geo)

// This workgroup's units, from (p.M, p.balanced, blockIdx, gridDim): declares `nu` (units of this workgroup; returns from the
// kernel if none), unit_tile0(i) (first tile of unit i) and unit_ntt(i) (its tiles, 0 past the last unit).  TT: the most tiles
// a unit may have.  Round-robin (p.balanced == 0, only where RR): 64-token units, unit i of workgroup b is number
// b + i * gridDim.  Balanced: workgroup b owns the contiguous tile range [T b / G, T (b + 1) / G) and walks it in equal units of
// <= TT tiles.  A macro, not a struct: as a force-inlined struct (by value or by reference, forced or left to the inliner) the
// same arithmetic reaches the back end in another order — two scalar operands swapped in mlp384_kernel, four instructions
// re-ordered in mlp192_kernel — while this text compiles to the instruction streams the three kernels had when each carried its
// own copy.  Uses `p` (MlpArgs) of the kernel it is written in.
#define MLP_UNIT_SCHEDULE(TT, RR)                                                                                       \
    const long long ntiles = (p.M + 15) >> 4;                                                                           \
    const long long t_beg = ntiles * blockIdx.x / gridDim.x, t_end = ntiles * (blockIdx.x + 1) / gridDim.x;             \
    const int n_own = (int)(t_end - t_beg);                                                                             \
    const long long nfix = (ntiles + (TT) - 2) / ((TT) - 1);                 /* 64-token units */                       \
    const int nu = (!(RR) || p.balanced) ? (n_own + (TT) - 1) / (TT)                                                    \
                                         : (int)((nfix - (long long)blockIdx.x + gridDim.x - 1) / gridDim.x);           \
    if (nu <= 0) return;                                                                                                \
    auto unit_tile0 = [&](int i) -> long long {                                                                         \
        if (!(RR) || p.balanced) return t_beg + (long long)n_own * i / nu;                                              \
        return min(((long long)blockIdx.x + (long long)i * gridDim.x) * ((TT) - 1), ntiles);                            \
    };                                                                                                                  \
    auto unit_ntt = [&](int i) -> int {                                                                                 \
        if (i >= nu) return 0;                                                                                          \
        if (!(RR) || p.balanced) return (int)(unit_tile0(i + 1) - unit_tile0(i));                                       \
        return (int)min((long long)((TT) - 1), ntiles - unit_tile0(i));                                                 \
    }

// FMA: both plans prove |z * m| < 2^53 (one fused rounding == the reference's two), else multiply and add separately.
// Both plans prove |z * c| < 2^31 (the host refuses the kernel otherwise); |cm|, |cr| < 2^9 (host-checked) for rq_fast.
//
// Units and balance.  The token axis is cut into tiles of 16.  A unit costs one pass over both weight matrices whatever its
// size (measured, one unit per CU: 29.8 / 31.9 / 34.2 / 37.2 / 44.3 us for 1..5 tiles), so units are as large as the LDS
// allows and as few as possible.  Two schedules, chosen by the host: 64-token units dealt round-robin, or — when that
// needs one more round than the work — workgroup b owns the contiguous tile range [T b / G, T (b + 1) / G) and walks it in
// units of <= 5 tiles (TT = 5: hidden 120 KB + activations 30 KB + table lines 4 KB of LDS): DeiT-S at batch 256 is
// 3152 tiles on 256 CUs = 12.3 per CU, three units of (5,) 4, 4 tiles instead of 3.08 -> 4 rounds of 64-token units.
// The unit body is instantiated for 4 and for 5 tiles (a unit with fewer tiles runs the 4-tile body on clamped rows).
//
// Software pipeline of both GEMM phases (pinned with scheduling fences: left alone the scheduler sinks every load to just
// before its first use and each step waits out a full LDS / L2 latency with the matrix pipe idle — measured 2.5-3.5x the
// MFMA time; hoisted to the top of the unrolled phase they are all live at once and spill): step s issues the weight
// fragments of step s + WD and the activation fragments of step s + 1, then its own MFMAs.
//
// The body is ivit_mlp_body.h, included into each entry point: the kernels keep their names (profilers and bench tools sort
// by them) and each compiles as if the body were written out in it.
template <bool FMA>
__global__ __launch_bounds__(Mlp384Geo::THREADS, Mlp384Geo::WAVES * Mlp384Geo::WG_PER_CU / 4) void mlp384_kernel(MlpArgs p) {
    typedef Mlp384Geo G;
    constexpr bool LNH = false;
#include "ivit_mlp_body.h"
}
template <bool FMA>
__global__ __launch_bounds__(Mlp192Geo::THREADS, Mlp192Geo::WAVES * Mlp192Geo::WG_PER_CU / 4) void mlp192_kernel(MlpArgs p) {
    typedef Mlp192Geo G;
    constexpr bool LNH = false;
#include "ivit_mlp_body.h"
}
template <bool FMA>
__global__ __launch_bounds__(Mlp256Geo::THREADS, Mlp256Geo::WAVES * Mlp256Geo::WG_PER_CU / 4) void mlp256_kernel(MlpArgs p) {
    typedef Mlp256Geo G;
    constexpr bool LNH = false;
#include "ivit_mlp_body.h"
}
// The LayerNorm-headed form of the two ViT widths (ivit_mlp_body.h, LNH): norm2 + qact3 + the Mlp + the residual QuantAct
// (vit_quant.py:139-142, layers_quant.py:144-153) in one launch.  Kernels of their own names, not a second template parameter of
// the two above: those keep their symbols (profilers, bench tools and tests/test_mlp192_cpu.py find them by name)
template <bool FMA>
__global__ __launch_bounds__(Mlp384Geo::THREADS, Mlp384Geo::WAVES * Mlp384Geo::WG_PER_CU / 4) void mlp384ln_kernel(MlpArgs p) {
    typedef Mlp384Geo G;
    constexpr bool LNH = true;
#include "ivit_mlp_body.h"
}
template <bool FMA>
__global__ __launch_bounds__(Mlp192Geo::THREADS, Mlp192Geo::WAVES * Mlp192Geo::WG_PER_CU / 4) void mlp192ln_kernel(MlpArgs p) {
    typedef Mlp192Geo G;
    constexpr bool LNH = true;
#include "ivit_mlp_body.h"
}
// width 128: the body once per requant form (FMA here is rq_magic's RQ: 0 or 2), and the kernel that picks between them — every
// workgroup reads the 640 multipliers and biases once and asks whether |z c| < 2^31 holds for all of them, with |z| <= K * 2^14
// + |bias| (the bound swin_mlp_rs_kernel uses)
template <int FMA>
__device__ __forceinline__ void mlp128_body(const MlpArgs &p) {
    typedef Mlp128Geo G;
    constexpr bool LNH = false;
#include "ivit_mlp_body.h"
}
__global__ __launch_bounds__(Mlp128Geo::THREADS, Mlp128Geo::WAVES * Mlp128Geo::WG_PER_CU / 4) void mlp128_kernel(MlpArgs p) {
    typedef Mlp128Geo G;
    bool wide = false;
    for (int ch = threadIdx.x; ch < G::HD + G::C; ch += G::THREADS) {
        const bool first = ch < G::HD;
        const int n = first ? ch : ch - G::HD;
        const ivit_dyadic d = reinterpret_cast<const ivit_dyadic *>(first ? p.cq1 : p.cq2)[n];
        const int32_t *b = first ? p.b1 : p.b2;
        const double zmax = (double)(first ? G::C : G::HD) * 16384.0 + fabs((double)(b ? b[n] : 0));
        wide |= !rq_magic_safe(d.m * d.r, zmax);
    }
    if (__syncthreads_or(wide)) mlp128_body<2>(p);
    else mlp128_body<0>(p);
}
