// ivit_attnmap.h — the class token's attention probabilities (include/ivit_attnmap.h): row 0 of IntSoftmax's output of one block
// (vit_quant.py:74, 16 bit, scale 2^-15) for every image and head, from the q and k a block's qkv launch has left, and their fp32
// map over the patches.  The fused attention kernels keep scores and probabilities in registers; this is the one row a caller
// may see, as a launch of its own beside them.
//
// attn_cls_probs_kernel: one wavefront per (image, head), four per 256-thread block, no block barrier (whole wavefronts beyond
// B * H leave at once).  Lane l owns the keys l, l + 64, ...:
//   pass 1  acc = q[bh, 0, :] . k[bh, j, :] in int32 (k in 16-byte pieces, the q piece is the same address on every lane),
//           sc8 = clamp8(rne(fl64(acc * c))) with rq_c — the general form, any multiplier —, staged in LDS as fp32; the row's
//           integer maximum rides along and is reduced over the wavefront;
//   pass 2  the lane's own entries again: requotient_c, shift_exp_c against the maximum, the exp value back into the same LDS word;
//   then the wave barrier, torch_order_sum32 on lanes 0..31 (both halves compute it, as shiftmax_kernel's do), recip_factor and
//   floorf((e * F) * 2^-16): the statement sequence of shiftmax_kernel (ivit_elementwise.h) at out_bits = 16, helper for helper.
// LDS: T floats per wavefront.  p_cls rows abut and T is odd in every real model: 2-byte stores, one per element.
//
// attn_map_f32_kernel: one thread per output element, patch columns j = 1 .. T - 1 only.
//   MEAN = false  out[r, h, j - 1] = fl32(p) * 2^-15 (p <= 32768: exact)
//   MEAN = true   S = sum_h p[r, h, j] in int32 (H <= 511: below 2^24, exact in fp32), out[r, j - 1] = fl32(S) / fl32(H * 32768):
//                 the IEEE division of the compiler (no fast-math), one rounding.
#pragma once
#include "../../include/ivit_attnmap.h"

#define ATTNMAP_MAX_T 1024
#define ATTNMAP_MAX_DH 128
#define ATTNMAP_MAX_H 511        // H * 32768 < 2^24

__device__ __forceinline__ int attnmap_dot16(v4i a, v4i b) {
    int acc = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc += (int)(int8_t)((unsigned)a[d] >> (8 * e)) * (int)(int8_t)((unsigned)b[d] >> (8 * e));
    return acc;
}

__global__ __launch_bounds__(256) void attn_cls_probs_kernel(const int8_t *__restrict__ q, const int8_t *__restrict__ k, double c, float s,
                                                             uint16_t *__restrict__ p_cls, int BH, int T, int dh) {
    extern __shared__ __attribute__((aligned(16))) char dsmem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *er = reinterpret_cast<float *>(dsmem) + (size_t)wave * T;
    const long long bh = (long long)blockIdx.x * 4 + wave;
    if (bh >= BH) return;
    const int nch = dh >> 4;
    const v4i *qp = reinterpret_cast<const v4i *>(q + (size_t)bh * T * dh);         // row 0 of this (image, head)
    const int8_t *kp = k + (size_t)bh * T * dh;
    int qmax = -128;
    for (int j = lane; j < T; j += 64) {
        const v4i *kr = reinterpret_cast<const v4i *>(kp + (size_t)j * dh);
        int acc = 0;
        for (int ch = 0; ch < nch; ++ch) acc += attnmap_dot16(qp[ch], kr[ch]);
        const int sc8 = rq_c((double)acc, c, -128, 127);
        er[j] = (float)sc8;
        qmax = max(qmax, sc8);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) qmax = max(qmax, __shfl_xor(qmax, o));
    const RcpC sr = rcp_prepare(s);
    const float mx = requotient_c((float)qmax, sr);
    const float x0 = floorf(-1.0f / s);
    const RcpC x0r = rcp_prepare(x0);
    const float nx0 = 15.0f * x0;
    for (int j = lane; j < T; j += 64) {
        const float xt = requotient_c(er[j], sr);
        er[j] = shift_exp_c(xt - mx, x0r, nx0, 15);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const float S = torch_order_sum32(T, lane & 31, [&](int idx) { return er[idx]; });
    const float F = recip_factor(S);
    const float div = ldexpf(1.0f, -16);            // out_bits = 16
    uint16_t *op = p_cls + (size_t)bh * T;
    for (int j = lane; j < T; j += 64) op[j] = (uint16_t)(int)floorf((er[j] * F) * div);
}

template <bool MEAN>
__global__ __launch_bounds__(256) void attn_map_f32_kernel(const uint16_t *__restrict__ p_cls, long long rows, int H, int T, float *__restrict__ out) {
    const int np = T - 1;
    const long long total = rows * (MEAN ? 1 : H) * np;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long rh = i / np;                    // MEAN: the row; else row * H + head
    const int j = (int)(i - rh * np) + 1;
    if constexpr (MEAN) {
        const uint16_t *pr = p_cls + (size_t)rh * H * T + j;
        int S = 0;
        for (int h = 0; h < H; ++h) S += (int)pr[(size_t)h * T];
        out[i] = (float)S / (float)(H * 32768);
    } else {
        out[i] = (float)p_cls[(size_t)rh * T + j] * 3.0517578125e-05f;      // 2^-15
    }
}
