// ivit_topk.h — top-k of the dequantised head outputs, with a stated order (include/ivit.h, ivit_logits_topk).
//
// The only thing the reference does with the model's output is validate() (quant_train.py:314-351): the head's int32
// accumulators times the per-class head scale (quant_modules.py:96-97: F.linear(...) * bias_scaling_factor, returned
// unchanged by vit_quant.py:278-282 / swin_quant.py:560-564), then top-1 / top-5 against the labels.
//
//   value   v[b, c] = fl32(fl32(acc[b, c]) * scale[c]): one v_cvt_f32_i32 (RNE) and one v_mul_f32.  There is no addition
//           here to contract with, and the library is built -ffp-contract=off.  `val` holds exactly these bits, -0.0 included.
//   order   descending by value; -0.0 and +0.0 compare equal; equal values by ascending class index.  Row b of idx is the
//           first k entries of np.lexsort((arange(ncls), -(v[b] + 0.0))).
//   Non-finite scale[c] is OUTSIDE the contract (no frozen model has one): a NaN product has no place in the order above.
//
// One wavefront per image, four images per 256-thread block, no LDS and no barrier.  A class becomes one 64-bit key:
// the order-preserving unsigned image of the fp32 value (zero canonicalised) in the high word, 0xFFFFFFFF - c in the low
// word, so ONE unsigned maximum gives value order and tie-break at once, and keys are distinct.  Round j takes the
// wave-wide maximum of the keys BELOW round j - 1's winner (distinct keys: that is "every class not yet taken"); lane j
// keeps the winner's class and, after the k rounds, lanes 0 .. k-1 recompute their value from memory and store (idx, val)
// with two coalesced vector stores.
//   REG = true  (ncls <= 1024): lane l holds classes l, l + 64, ... as TOPK_PER_LANE keys in registers; the row is read once.
//   REG = false (any ncls):     every round rescans the row from memory (L2-resident after the first pass).
#pragma once
#include "ivit_device.h"

#define TOPK_MAX_K 16
#define TOPK_PER_LANE 16                          // register form: classes per lane
#define TOPK_REG_CLASSES (64 * TOPK_PER_LANE)     // 1024

__device__ __forceinline__ float topk_value(int acc, float scale) { return __fmul_rn((float)acc, scale); }

// 0 is no class's key (the low word of a real key is 0xFFFFFFFF - c > 0 for c < 2^31): it stands for "nothing"
__device__ __forceinline__ unsigned long long topk_key(int acc, float scale, int c) {
    unsigned u = __float_as_uint(topk_value(acc, scale));
    u = u == 0x80000000u ? 0u : u;                                   // -0.0 ties +0.0
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);                  // unsigned order == float order
    return ((unsigned long long)u << 32) | (0xFFFFFFFFu - (unsigned)c);
}

__device__ __forceinline__ unsigned long long topk_wave_max(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

template <bool REG>
__global__ __launch_bounds__(256) void logits_topk_kernel(const int *__restrict__ logits, const float *__restrict__ scale, int batch,
                                                          int ncls, int k, int *__restrict__ idx, float *__restrict__ val) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= batch) return;                                          // whole wavefronts leave: nothing below synchronises a block
    const int *row = logits + (size_t)b * ncls;

    unsigned long long keys[TOPK_PER_LANE];
    if constexpr (REG) {
#pragma unroll
        for (int i = 0; i < TOPK_PER_LANE; ++i) {
            const int c = i * 64 + lane;
            keys[i] = c < ncls ? topk_key(row[c], scale[c], c) : 0ull;
        }
    }

    unsigned long long last = ~0ull;                                 // above every key
    int mine = 0;                                                    // lane j: the class of rank j
    for (int j = 0; j < k; ++j) {
        unsigned long long best = 0ull;
        if constexpr (REG) {
#pragma unroll
            for (int i = 0; i < TOPK_PER_LANE; ++i) {
                const unsigned long long cand = keys[i] < last ? keys[i] : 0ull;
                best = cand > best ? cand : best;
            }
        } else {
            for (int c = lane; c < ncls; c += 64) {
                const unsigned long long key = topk_key(row[c], scale[c], c);
                const unsigned long long cand = key < last ? key : 0ull;
                best = cand > best ? cand : best;
            }
        }
        last = topk_wave_max(best);                                  // k <= ncls: a class is left, last != 0
        if (lane == j) mine = (int)min(0xFFFFFFFFu - (unsigned)last, (unsigned)ncls - 1u);      // a real key's class is < ncls already
    }
    if (lane < k) {
        idx[(size_t)b * k + lane] = mine;
        if (val) val[(size_t)b * k + lane] = topk_value(row[mine], scale[mine]);
    }
}
