// ivit_classmap.h — class-activation maps of a Swin (include/ivit_classmap.h): the per-token evidence for a class, the head's weight
// row against every final-stage token.  A Swin ends in norm -> qact2 -> average pool -> qact3 -> head (swin_quant.py:551-564), and
// qact2 is applied to every token, so the tokens tok8 [B, L, C] are int8 integers on ONE scale and
//   cam32[b, j, t] = sum_c head_w[idx[b, j], c] * tok8[b, t, c]
// is an int32 with no rounding anywhere: |cam32| <= 128 * 127 * C < 2^24 for C <= 1024, so its fp32 form is exact too.
//
// class_map_kernel<MAP>: one wavefront per (image, class slot), four per 256-thread block, no block barrier, no LDS (whole wavefronts
// beyond B * k leave at once).  The wavefront reads its class index from device memory — the top-k launch in front of it wrote it, or
// the caller did — and judges it BEFORE it forms an address: an index outside [0, num_classes) reads class 0's row and stores zeros
// (and NaN) instead.  Lane l owns the tokens l, l + 64, ...: the dot product over C in 16-byte pieces of the token row against
// the weight row's piece, the same address on every lane, four v_dot4_i32_i8 per piece (signed x signed, int32, no clamp: the
// integers of the sum above in any order).  MAP = true also stores map32 = fl32(fl32(cam32) * class_scale[class]) from the same
// registers: one conversion, exact, and one multiply (-ffp-contract=off: nothing to fuse with), v[b, c] of ivit_logits_topk.
#pragma once
#include "../../include/ivit_classmap.h"

#define CLASSMAP_MAX_C 1024      // 128 * 127 * C < 2^24
#define CLASSMAP_MAX_K 16        // TOPK_MAX_K: the top-k launch in front fills at most that many slots

template <bool MAP>
__global__ __launch_bounds__(256) void class_map_kernel(const int8_t *__restrict__ tok8, const int8_t *__restrict__ head_w,
                                                        const int32_t *__restrict__ idx, const float *__restrict__ class_scale,
                                                        int32_t *__restrict__ cam32, float *__restrict__ map32, int BK, int k, int L, int C,
                                                        int num_classes) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long bk = (long long)blockIdx.x * 4 + wave;      // (image, class slot)
    if (bk >= BK) return;
    const int cls = idx[bk];
    const bool valid = (unsigned)cls < (unsigned)num_classes;
    const int row = valid ? cls : 0;                             // the guard: no address is formed from an index out of range
    const v4i *wp = reinterpret_cast<const v4i *>(head_w + (size_t)row * C);
    const int8_t *tp = tok8 + (size_t)(bk / k) * L * C;
    const int nch = C >> 4;
    float sc = 0.f;
    if constexpr (MAP) sc = class_scale[row];
    for (int t = lane; t < L; t += 64) {
        const v4i *tr = reinterpret_cast<const v4i *>(tp + (size_t)t * C);
        int acc = 0;
        for (int ch = 0; ch < nch; ++ch) {
            const v4i a = wp[ch], b = tr[ch];
#pragma unroll
            for (int d = 0; d < 4; ++d) acc = __builtin_amdgcn_sdot4(a[d], b[d], acc, false);
        }
        const size_t o = (size_t)bk * L + t;
        cam32[o] = valid ? acc : 0;
        if constexpr (MAP) map32[o] = valid ? (float)acc * sc : __uint_as_float(0x7fc00000u);
    }
}
