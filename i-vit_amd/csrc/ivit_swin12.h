// ivit_swin12.h — the Swin windowed attention at window 12 (patch4_window12_384 family); shares the conventions and
// helpers of window_attention_kernel (ivit_swin.h).  The kernel is a template on the window (12 only) so that the compiler
// emits it among the template instantiations, after the ViT kernels: adding it moved those by the 30 KB of its code
// otherwise, and the DeiT-S step measured 0.4 % slower with them moved.
#pragma once
#include "ivit_device.h"
#include "ivit_swin.h"

// ---------------------------------------------------------------------------
// The same operator for window 12x12 (N = 144 tokens, 5 key tiles of 32 with keys 144..159 padding), head dim 32.
// A block = ONE head x up to p.wpb windows, 5 wavefronts: wave w owns queries 32w .. 32w + 31 of each window (a 160 x 160
// score tile does not fit one wavefront's registers).  The head's [144][144] bias slab is staged once per block; per window
// the block stages K and V (160 rows x 32 B each, rows >= 144 zero; double-buffered, one barrier per window) and the
// window's mask regions in LDS, Q fragments come straight from global.  Same arithmetic as the window-7 kernel:
//   S^T = K Q^T      5 x v_mfma_i32_32x32x32_i8: lane holds query (lane & 31) and, in key tile kt, register r,
//                    key 32kt + 8(r>>2) + 4*half + (r&3) -> a query's 144 scores sit in 2 lanes x 72 registers
//   a   = clamp8(rq(clamp8(rq(S, dy_qk)), dy_a) + relb[h][q][k])  (+ shift mask, SURVEY A.8, as in the window-7 kernel)
//   P   = Shiftmax_8bit(a) with torch's row sum for n = 144 (ivit_device.h torch_order_sum32): accumulator sub = k mod 32
//         adds keys sub, 32+sub, 64+sub, 96+sub and, for sub < 8, 128+sub, 136+sub; p[l] = ((a[l]+a[8+l])+a[16+l])+a[24+l];
//         S = p[0] + ... + p[7].  Register r of a lane is accumulator 8(r>>2) + 4*half + (r&3) in every key tile, and
//         tile 4's registers e and 4+e are keys 128+4*half+e and 136+4*half+e: accumulators and p[4*half + e] are
//         lane-local, only the 8-term tail crosses the two halves
//   O^T = V^T P^T    P <= 128: two MFMAs per key tile, B = P - 64 and B = 64 (padding keys: P - 64 = 0, V rows 0)
struct WinAttn12Args {
    const int8_t *qkv;      // [B, R, R, 3, heads, 32]
    int8_t *ctx;            // [B, R*R, heads*32]
    const int16_t *relb;    // [heads, 144, 144], 16-byte aligned
    int B, R, shift, heads;
    int wpb;                // windows per block
    ivit_dyadic dy_qk, dy_a, dy_pv;
    float s;
};
#define WA12_THREADS 320
#define WA12_KV 5120                               // 160 rows x 32 B
#define WA12_K (144 * 144 * 2)                     // 41472: bias slab [144][144] int16 at 0
#define WA12_REG (WA12_K + 4 * WA12_KV)            // 61952: 2 buffers x (K, V)
#define WA12_TA (WA12_REG + 2 * 160)               // 62272: 2 buffers x 160 mask regions
#define WA12_TX (WA12_TA + 512)                    // 62784: rq(v, dy_a), v = -128..127
#define WA12_SMEM (WA12_TX + 1024)                 // 63808: fl(fl(a*s)/s)

template <int WIN>
__global__ __launch_bounds__(WA12_THREADS, 3) void window_attention12_kernel(WinAttn12Args p) {
    static_assert(WIN == 12, "window 12 only");
    extern __shared__ __attribute__((aligned(16))) char sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int16_t *sRel = reinterpret_cast<const int16_t *>(sm);
    int16_t *sTa = reinterpret_cast<int16_t *>(sm + WA12_TA);
    float *sTx = reinterpret_cast<float *>(sm + WA12_TX);
    const int R = p.R, nw = R / 12, C = p.heads * 32;
    const long long nwin = (long long)p.B * nw * nw;
    // block -> (window group, head) as in the window-7 kernel: the heads of one window group on one XCD
    const int xcd = (int)(blockIdx.x & 7), bq = (int)(blockIdx.x >> 3);
    const int head = bq % p.heads;
    const long long w0 = ((long long)(bq / p.heads) * 8 + xcd) * p.wpb;
    if (w0 >= nwin) return;                                 // padding blocks of the last group of 8 (whole block)
    const float s = p.s;
    const RcpC sr = rcp_prepare(s);
    {   // the head's bias slab: 2592 pieces of 16 B, every load issued before the first store
        constexpr int NI = (2592 + WA12_THREADS - 1) / WA12_THREADS;
        const v4i *rb = reinterpret_cast<const v4i *>(p.relb + (long long)head * 20736);
        v4i t[NI];
#pragma unroll
        for (int u = 0; u < NI; ++u) if (tid + u * WA12_THREADS < 2592) t[u] = rb[tid + u * WA12_THREADS];
#pragma unroll
        for (int u = 0; u < NI; ++u) if (tid + u * WA12_THREADS < 2592) reinterpret_cast<v4i *>(sm)[tid + u * WA12_THREADS] = t[u];
    }
    if (tid < 256) {
        const double ca = p.dy_a.m * p.dy_a.r;
        sTa[tid] = (int16_t)(int)__builtin_rint((double)(tid - 128) * ca);
        sTx[tid] = requotient_c((float)(tid - 128), sr);
    }
    if (tid < 128) {                                        // padding rows 144..159 of both K / V buffers: zero, once
        const int kvb = tid >> 5, row = 144 + ((tid & 31) >> 1), hh = tid & 1;
        *reinterpret_cast<v4i *>(sm + WA12_K + kvb * WA12_KV + row * 32 + hh * 16) = v4i{0, 0, 0, 0};
    }
    const double c_qk = p.dy_qk.m * p.dy_qk.r, c_pv = p.dy_pv.m * p.dy_pv.r;
    const float x0 = floorf(-1.0f / s), nx0 = 15.0f * x0;
    const RcpC x0r = rcp_prepare(x0);
    const v4i c64 = {0x40404040, 0x40404040, 0x40404040, 0x40404040};
    const int q = wave * 32 + l31;                          // this lane's query (>= 144: padding)
    const bool qlive = q < 144;
    const int qq = qlive ? q : 143;

#pragma unroll 1
    for (int it = 0; it < p.wpb; ++it) {
        const long long wlin = w0 + it;
        if (wlin >= nwin) break;                            // uniform over the block
        const int buf = it & 1;
        char *sK = sm + WA12_K + buf * 2 * WA12_KV, *sV = sK + WA12_KV;
        unsigned char *sReg = reinterpret_cast<unsigned char *>(sm + WA12_REG + buf * 160);
        const int win = (int)(wlin % (nw * nw)), b = (int)(wlin / (nw * nw));
        const int wi = win / nw, wj = win - wi * nw;
        auto tok_off = [&](int n) -> long long {             // natural token index of window token n
            const int wy = n / 12, wx = n - wy * 12;
            int y = wi * 12 + wy + p.shift, x = wj * 12 + wx + p.shift;
            y = y >= R ? y - R : y;
            x = x >= R ? x - R : x;
            return ((long long)b * R + y) * R + x;
        };
        const bool masked = p.shift > 0 && (wi == nw - 1 || wj == nw - 1);
        // ---- K, V rows of the window -> LDS (144 tokens x {K, V} x 2 pieces of 16 B), mask regions, this wave's Q
        for (int i = tid; i < 576; i += WA12_THREADS) {
            const int n = i >> 2, kv = (i >> 1) & 1, hh = i & 1;
            const v4i v = *reinterpret_cast<const v4i *>(p.qkv + tok_off(n) * (3 * C) + (1 + kv) * C + head * 32 + hh * 16);
            *reinterpret_cast<v4i *>((kv ? sV : sK) + n * 32 + hh * 16) = v;
        }
        if (tid < 144) {
            const int wy = tid / 12, wx = tid - wy * 12, ys = wi * 12 + wy, xs = wj * 12 + wx;
            const int ry = ys < R - 12 ? 0 : (ys < R - p.shift ? 1 : 2), rx = xs < R - 12 ? 0 : (xs < R - p.shift ? 1 : 2);
            sReg[tid] = (unsigned char)(ry * 3 + rx);
        }
        v4i qf = {0, 0, 0, 0};
        if (qlive) qf = *reinterpret_cast<const v4i *>(p.qkv + tok_off(q) * (3 * C) + head * 32 + half * 16);
        __syncthreads();     // this window's K / V / regions (and, on the first pass, the slab and tables) are in place;
                             // every wave is done with the window before last, whose buffer the next pass refills

        v16i_sw acc[5];
#pragma unroll
        for (int kt = 0; kt < 5; ++kt) {
            const v4i kf = *reinterpret_cast<const v4i *>(sK + (kt * 32 + l31) * 32 + half * 16);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[kt][r] = 0;
            acc[kt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(kf, qf, acc[kt], 0, 0, 0);
        }
        // valid keys: tiles 0..3 all 16 registers, tile 4 registers 0..7 (keys 128..143)
        const int regq = sReg[qq];
        const int16_t *relq = sRel + qq * 144;
        float f[72];
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < 72; ++i) {
            const int kt = i >> 4, r = i & 15;
            const int key = 32 * kt + 8 * (r >> 2) + 4 * half + (r & 3);
            const int v = min(max(__double2loint((double)acc[kt][r] * c_qk + RQ_MAGIC), -128), 127);
            const int a = min(max((int)sTa[v + 128] + (int)relq[key], -128), 127);
            float xt;
            if (masked) {
                float X = (float)a * s;
                X = X + ((sReg[key] != regq) ? -100.0f : 0.0f);
                xt = lean_div(X, sr);
            } else {
                xt = sTx[a + 128];
            }
            f[i] = xt;
            mx = fmaxf(mx, xt);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
#pragma unroll
        for (int i = 0; i < 72; ++i) f[i] = shift_exp_nonpos(f[i] - mx, x0r, nx0, 15);
        // torch-order row sum (n = 144): p[4*half + e] lane-local, then p[0..3] (half 0) and p[4..7] (half 1) in order
        float pl[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float ak[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) ak[k] = ((f[4 * k + e] + f[16 + 4 * k + e]) + f[32 + 4 * k + e]) + f[48 + 4 * k + e];
            ak[0] = (ak[0] + f[64 + e]) + f[68 + e];
            pl[e] = ((ak[0] + ak[1]) + ak[2]) + ak[3];
        }
        const float lo = __shfl((((pl[0] + pl[1]) + pl[2]) + pl[3]), l31);     // half 0's p[0..3]
        const float hi = (((lo + pl[0]) + pl[1]) + pl[2]) + pl[3];                 // meaningful on half 1
        const float S = __shfl(hi, l31 + 32);
        const float F16 = recip_factor(S) * 5.9604644775390625e-08f;            // * 2^-24 (exact scaling)
        // probabilities (0..128) -> B fragments P - 64 in the lane's own key order; V^T fragments in the same order
        v16i_sw o;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = 0;
#pragma unroll
        for (int kt = 0; kt < 5; ++kt) {
            v4i pf, vf;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                unsigned pw = 0, vw = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = w * 4 + e, i = kt * 16 + r;
                    const int P = (kt < 4 || r < 8) ? (int)(f[i < 72 ? i : 71] * F16) : 64;   // >= 0: truncation is the floor
                    pw |= (unsigned)((P - 64) & 0xff) << (8 * e);
                    const int key = 32 * kt + e + 8 * w + 4 * half;
                    vw |= (unsigned)(unsigned char)sV[key * 32 + l31] << (8 * e);
                }
                pf[w] = (int)pw;
                vf[w] = (int)vw;
            }
            o = __builtin_amdgcn_mfma_i32_32x32x32_i8(vf, pf, o, 0, 0, 0);
            o = __builtin_amdgcn_mfma_i32_32x32x32_i8(vf, c64, o, 0, 0, 0);
        }
        // O^T[d][query]: lane = query, register quad g -> d = 8g + 4*half + (0..3)
        unsigned W[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            int ob[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                ob[e] = min(max(__double2loint((double)o[g * 4 + e] * c_pv + RQ_MAGIC), -128), 127);
            unsigned w01 = __builtin_amdgcn_perm((unsigned)ob[1], (unsigned)ob[0], 0x0c0c0400u);
            unsigned w23 = __builtin_amdgcn_perm((unsigned)ob[3], (unsigned)ob[2], 0x0c0c0400u);
            W[g] = __builtin_amdgcn_perm(w23, w01, 0x05040100u);
        }
        auto s02 = __builtin_amdgcn_permlane32_swap(W[0], W[2], false, false);
        auto s13 = __builtin_amdgcn_permlane32_swap(W[1], W[3], false, false);
        const v4i outv = {(int)s02[0], (int)s02[1], (int)s13[0], (int)s13[1]};   // d = 16*half .. +16
        if (qlive) *reinterpret_cast<v4i *>(p.ctx + tok_off(q) * C + head * 32 + half * 16) = outv;
    }
}

