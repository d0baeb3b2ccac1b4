// ivit_score.h — rank and negative log-likelihood of the label among the dequantised head outputs (include/ivit_eval.h,
// ivit_logits_score): what validate() needs for Loss / Acc@1 / Acc@5 (quant_train.py:335-339), one launch per batch.
//
//   value   v[b, c] = topk_value(acc[b, c], scale[c]), the value of ivit_topk.h: one conversion, one multiply.
//   rank    the number of classes c with topk_key(c) > topk_key(label): the keys of ivit_topk.h, so the order (descending value,
//           -0.0 == +0.0, ties by ascending class) cannot drift from the top-k's.  Keys are distinct: rank is the label's place.
//   nll     d = (double)v, m = max(d): log(sum exp(d - m)) - (d[label] - m) in fp64.  The maximum is taken in fp32 (the
//           conversion is monotone and exact, so it is the fp64 maximum; a -0.0 maximum beside a +0.0 changes no term).
//   A label outside [0, ncls) is replaced by class 0 for every address, and the stores write INT32_MAX / NaN instead.
//
// Geometry of logits_topk_kernel: one wavefront per image, four images per 256-thread block, no LDS and no barrier; three
// wave reductions through __shfl_xor (maximum, sum, count) and lane 0 stores.
//   REG = true  (ncls <= 1024): lane l holds classes l, l + 64, ... in registers; the row is read once.
//   REG = false (any ncls):     two passes over the row (maximum, then sum and count; L2-resident after the first).
#pragma once
#include "../../include/ivit_eval.h"
#include "ivit_topk.h"

__device__ __forceinline__ float score_wave_max(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    return v;
}

__device__ __forceinline__ double score_wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ int score_wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <bool REG>
__global__ __launch_bounds__(256) void logits_score_kernel(const int *__restrict__ logits, const float *__restrict__ scale,
                                                           const long long *__restrict__ labels, int batch, int ncls,
                                                           int *__restrict__ rank, double *__restrict__ nll) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= batch) return;                                          // whole wavefronts leave: nothing below synchronises a block
    const int *row = logits + (size_t)b * ncls;

    const long long label = labels[b];                               // wave-uniform
    const bool valid = label >= 0 && label < ncls;
    const int lc = valid ? (int)label : 0;                           // the only class an address is formed from: always in the row
    const float lv = topk_value(row[lc], scale[lc]);
    const unsigned long long lkey = topk_key(row[lc], scale[lc], lc);

    int acc[TOPK_PER_LANE];
    float sc[TOPK_PER_LANE];
    float m = lv;                                                    // a value of the row: the maximum needs no "minus infinity"
    if constexpr (REG) {
#pragma unroll
        for (int i = 0; i < TOPK_PER_LANE; ++i) {
            const int c = i * 64 + lane;
            acc[i] = c < ncls ? row[c] : 0;
            sc[i] = c < ncls ? scale[c] : 0.0f;
            m = c < ncls ? fmaxf(m, topk_value(acc[i], sc[i])) : m;
        }
    } else {
        for (int c = lane; c < ncls; c += 64) m = fmaxf(m, topk_value(row[c], scale[c]));
    }
    m = score_wave_max(m);

    const double dm = (double)m;
    double sum = 0.0;
    int above = 0;
    if constexpr (REG) {
#pragma unroll
        for (int i = 0; i < TOPK_PER_LANE; ++i) {
            const int c = i * 64 + lane;
            if (c < ncls) {
                above += topk_key(acc[i], sc[i], c) > lkey;
                if (nll) sum += exp((double)topk_value(acc[i], sc[i]) - dm);
            }
        }
    } else {
        for (int c = lane; c < ncls; c += 64) {
            const int a = row[c];
            const float s = scale[c];
            above += topk_key(a, s, c) > lkey;
            if (nll) sum += exp((double)topk_value(a, s) - dm);
        }
    }
    above = score_wave_sum(above);
    if (nll) sum = score_wave_sum(sum);                              // nll is a kernel argument: the branch is uniform

    if (lane == 0) {
        if (rank) rank[b] = valid ? above : 0x7FFFFFFF;
        if (nll) nll[b] = valid ? log(sum) - ((double)lv - dm) : __longlong_as_double(0x7FF8000000000000ll);
    }
}
