// ivit_features.h — the fp32 form of int8 features (include/ivit_features.h, ivit_features_f32): what forward_features returns in the
// reference (QuantAct's integer * scale, quant_modules.py:197-206), or the same rows at unit Euclidean length.  One launch per batch.
//
//   UNIT = false  out[b, c] = fl32(fl32(q) * scale): v_cvt_f32_i32 and one multiply (the library is built with -ffp-contract=off).
//   UNIT = true   ss = sum q^2 in int32 (dim <= 65536: at most 2^30), s = sqrt((double)ss), out[b, c] = fl32((double)q / s).
//                 The contract wants the CORRECTLY ROUNDED fp64 root.  sqrt() of the compiler is followed by one residual step,
//                 r = fma(-s, s, x) (the exact residual's rounding), s' = fma(r, 0.5 / s, s): from a root that is off by an ulp it
//                 gives the correctly rounded one, and it leaves a correctly rounded one alone (|r / 2s| < ulp / 2 then, and the root
//                 of a 31-bit integer is an fp64 number or far from a midpoint of two).  x = 0 is replaced by 1 before the root
//                 and every q is 0 then: a row of zeros gives +0.0, never NaN.  The fp64 division is IEEE (no fast-math).
//
// Geometry: one wavefront per row, four rows per 256-thread block, no LDS and no barrier.  Lane l takes the 16-byte chunks l,
// l + 64, ... of its row (dim is a multiple of 16 and rows are 16-byte aligned: one global_load_dwordx4 each) and stores them as four
// float4.  A lane whose chunk lies beyond the row loads nothing and adds nothing, but STAYS in the wavefront: all 64 lanes take
// part in the __shfl_xor sum.  Whole wavefronts beyond the batch leave at once.  UNIT reads the row twice (the second time from L2).
#pragma once
#include "../../include/ivit_features.h"

#define FEATURES_MAX_DIM 65536

__device__ __forceinline__ int features_byte(int w, int k) { return (int)(signed char)((unsigned)w >> (8 * k)); }

__device__ __forceinline__ int features_wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <bool UNIT>
__global__ __launch_bounds__(256) void features_f32_kernel(const int8_t *__restrict__ feat8, int batch, int dim, float scale,
                                                           float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= batch) return;                                          // whole wavefronts leave: nothing below synchronises a block
    const int4 *row = reinterpret_cast<const int4 *>(feat8 + (size_t)b * dim);
    float4 *orow = reinterpret_cast<float4 *>(out + (size_t)b * dim);
    const int nchunks = dim >> 4;

    double s = 1.0;
    if constexpr (UNIT) {
        int ss = 0;
        for (int c = lane; c < nchunks; c += 64) {
            const int4 v = row[c];
            const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int k = 0; k < 4; ++k) { const int q = features_byte(w[j], k); ss += q * q; }
        }
        ss = features_wave_sum(ss);                                  // wave-uniform from here
        const double x = ss ? (double)ss : 1.0;
        s = sqrt(x);
        s = fma(fma(-s, s, x), 0.5 / s, s);
    }
    for (int c = lane; c < nchunks; c += 64) {
        const int4 v = row[c];
        const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int q = features_byte(w[j], k);
                o[k] = UNIT ? (float)((double)q / s) : (float)q * scale;
            }
            orow[c * 4 + j] = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
}
