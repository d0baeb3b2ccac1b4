// ivit_preprocess.h — the reference's eval transform (utils/data_utils.py:82-92) on a RAGGED batch of uint8 HWC images, bit-exact
// with PIL: Resize(size, bicubic) + CenterCrop(crop) [+ ToTensor + Normalize + the input QuantAct] in ONE launch.
//
// PIL resamples uint8 images in 22-bit fixed point, horizontally first into a uint8 intermediate, then vertically
// (ImagingResample).  Per axis (input length `in`, output length `out`), all in double and in this operation order
// (-ffp-contract=off: no fma is formed):
//   scale = in / out; fs = max(scale, 1); support = 2 fs; ss = 1 / fs;
//   output index i: center = (i + 0.5) scale; xmin = max((int)(center - support + 0.5), 0);
//                   n = min((int)(center + support + 0.5), in) - xmin;
//                   w_j = f((j + xmin - center + 0.5) ss); ww = w_0 + w_1 + ... (ascending, from 0.0); w_j /= ww if ww != 0;
//                   k_j = (int)(w_j 2^22 +- 0.5)  (sign of w_j, truncating);
//   one pass: clamp((2^21 + sum_j pixel_j k_j) >> 22, 0, 255), int32, arithmetic shift.
// An axis whose length does not change is copied: here the one tap k = 2^22, (2^21 + p 2^22) >> 22 == p.
// Everything behind the coefficients is integer arithmetic: no fp32 anywhere in the resampling, and the vertical sum may be
// accumulated in any order.  tests/golden/pil_resize.npz (written by PIL itself) is the pin.
//
// Work shape.  The grid is ceil(crop / PIL_BAND) x B workgroups of PIL_THREADS: a workgroup owns one image and one band of
// PIL_BAND output rows, and walks the crop in chunks of at most PIL_CHUNK_COLS columns (one chunk at crop <= 256), so every
// LDS array has a size that depends on nothing.  Per chunk it builds the horizontal tap table (xmin, n, k_j of each column: one
// thread per column, once, never per pixel), then takes one of two forms, chosen per image from its size alone:
//   tiled      vertical tap count ksize_v = 2 ceil(support_v) + 1 <= PIL_TILE_ROWS (a down-scale up to 23.5).  The band's
//              vertical table is built once; the band is cut into sub-bands, each the most output rows whose taps reach at most
//              PIL_TILE_ROWS input rows (32 rows up to a down-scale of 2.8, fewer above: the height follows the vertical
//              scale); those input rows are staged in LDS and passed horizontally, for the chunk's columns, into a uint8 LDS tile; the
//              vertical pass out of the tile.
//   streaming  ksize_v > PIL_TILE_ROWS.  One thread per column; input rows arrive in ascending order, each is passed
//              horizontally in registers and added into the int32 LDS accumulators of the output rows whose taps cover it
//              (vertical coefficients evaluated per (input row, output row), uniform over the workgroup).
// Horizontal taps: a chunk is narrowed to PIL_HTAB_INTS / ksize_h columns so that its table fits; beyond ksize_h >
// PIL_HTAB_INTS (a down-scale above 1023, always inside the streaming form) the coefficients are evaluated per tap from the
// column's stored xmin, n and ww.
// Epilogues: uint8 HWC, or the 3 x 256 table of normalize_quantize_u8_kernel (same fp32 sequence) as a byte gather with the
// HWC -> CHW transpose: the cropped uint8 image never exists in HBM.  Plain byte stores.
#pragma once
#include "ivit_device.h"

#define PIL_THREADS 512
#define PIL_BAND 32
#define PIL_TILE_ROWS 96
#define PIL_CHUNK_COLS 256
#define PIL_HTAB_INTS 4096
#define PIL_TILE_BYTES (PIL_TILE_ROWS * PIL_CHUNK_COLS * 3)
// tiled form: input rows are staged in LDS by coalesced byte loads (every load independent of the others) before the taps read
// them; read straight from global memory the taps of a column are a chain of dependent, uncoalesced byte loads.  One row of a
// chunk is at most 3 ((cw + 3) (ksize_h - 1) / 4 + 1) < 13 KB (cw ksize_h <= PIL_HTAB_INTS), so at least two rows fit.
#define PIL_RAW_BYTES 32768
// htab | vk | hww | vww | hx hn | vx vn | tile (the streaming form's accumulators) | lut | raw
#define PIL_LDS_BYTES (PIL_HTAB_INTS * 4 + PIL_BAND * PIL_TILE_ROWS * 4 + PIL_CHUNK_COLS * 8 + PIL_BAND * 8 + \
                       2 * PIL_CHUNK_COLS * 4 + 2 * PIL_BAND * 4 + PIL_TILE_BYTES + 768 + PIL_RAW_BYTES)

struct PilAxis {
    double scale, support, ss;
    long long ksize;        // PIL's bound on n: 2 ceil(support) + 1; 1 for an axis that is copied
    int in;
    bool same;
};
struct PilTap { int xmin, n; double center; };

__device__ __forceinline__ double pil_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
    return 0.0;
}
__device__ __forceinline__ PilAxis pil_axis(int in, long long out) {
    PilAxis a;
    a.in = in;
    a.same = out == (long long)in;
    a.scale = (double)in / (double)out;
    const double fs = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = 2.0 * fs;
    a.ss = 1.0 / fs;
    a.ksize = a.same ? 1 : (long long)ceil(a.support) * 2 + 1;
    return a;
}
__device__ __forceinline__ PilTap pil_tap(const PilAxis &a, long long i) {
    PilTap t;
    if (a.same) { t.xmin = (int)i; t.n = 1; t.center = 0.0; return t; }
    t.center = ((double)i + 0.5) * a.scale;
    t.xmin = max((int)(t.center - a.support + 0.5), 0);
    t.n = min((int)(t.center + a.support + 0.5), a.in) - t.xmin;
    return t;
}
__device__ __forceinline__ double pil_weight(const PilAxis &a, const PilTap &t, int j) {
    return pil_bicubic(((double)(j + t.xmin) - t.center + 0.5) * a.ss);
}
__device__ __forceinline__ double pil_weight_sum(const PilAxis &a, const PilTap &t) {
    double ww = 0.0;
    for (int j = 0; j < t.n; ++j) ww += pil_weight(a, t, j);
    return ww;
}
__device__ __forceinline__ int pil_coeff(const PilAxis &a, const PilTap &t, double ww, int j) {
    if (a.same) return 1 << 22;
    double w = pil_weight(a, t, j);
    if (ww != 0.0) w /= ww;
    return w < 0.0 ? (int)(-0.5 + w * 4194304.0) : (int)(0.5 + w * 4194304.0);
}
// the whole tap row of output index i: k[0 .. n)
__device__ __forceinline__ PilTap pil_build(const PilAxis &a, long long i, int *k) {
    const PilTap t = pil_tap(a, i);
    const double ww = a.same ? 0.0 : pil_weight_sum(a, t);
    for (int j = 0; j < t.n; ++j) k[j] = pil_coeff(a, t, ww, j);
    return t;
}
__device__ __forceinline__ int pil_clip8(int acc) { return min(max(acc >> 22, 0), 255); }

template <bool NCHW>
__device__ __forceinline__ void pil_store(unsigned char *__restrict__ out, const signed char *lut, int b, int crop, int row, int col,
                                          int ch, int v) {
    if (NCHW) out[(((long long)b * 3 + ch) * crop + row) * crop + col] = (unsigned char)lut[ch * 256 + v];
    else out[(((long long)b * crop + row) * crop + col) * 3 + ch] = (unsigned char)v;
}

template <bool NCHW>
__global__ __launch_bounds__(PIL_THREADS) void pil_eval_kernel(const unsigned char *__restrict__ pixels,
                                                               const ivit_image_desc *__restrict__ desc, int size, int crop,
                                                               int nbands, float m0, float m1, float m2, float s0, float s1,
                                                               float s2, float qscale, unsigned char *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char dsmem[];
    int *htab = reinterpret_cast<int *>(dsmem);                           // [chunk column][ksize_h]
    int *vk = htab + PIL_HTAB_INTS;                                       // tiled: [band row][ksize_v]
    double *hww = reinterpret_cast<double *>(vk + PIL_BAND * PIL_TILE_ROWS);   // per chunk column, when htab does not hold the taps
    double *vww = hww + PIL_CHUNK_COLS;                                   // streaming: per sub-band row
    int *hx = reinterpret_cast<int *>(vww + PIL_BAND), *hn = hx + PIL_CHUNK_COLS;
    int *vx = hn + PIL_CHUNK_COLS, *vn = vx + PIL_BAND;
    unsigned char *tile = reinterpret_cast<unsigned char *>(vn + PIL_BAND);
    int *acc = reinterpret_cast<int *>(tile);
    signed char *lut = reinterpret_cast<signed char *>(tile + PIL_TILE_BYTES);
    unsigned char *raw = reinterpret_cast<unsigned char *>(lut) + 768;

    const int tid = threadIdx.x;
    const int b = blockIdx.x / nbands, band = blockIdx.x - b * nbands;
    const ivit_image_desc d = desc[b];
    const unsigned char *img = pixels + d.offset;
    const int H = d.h, W = d.w;
    // torchvision Resize(int) + CenterCrop: the rule of ivit_resize_center_crop_u8
    long long Hr, Wr;
    if (H <= W) { Hr = size; Wr = (long long)size * W / H; }
    else { Wr = size; Hr = (long long)size * H / W; }
    const long long top = (long long)__builtin_rint((double)(Hr - crop) / 2.0), left = (long long)__builtin_rint((double)(Wr - crop) / 2.0);
    const PilAxis ah = pil_axis(W, Wr), av = pil_axis(H, Hr);

    if (NCHW) {             // normalize_quantize_u8_kernel's table, the same fp32 sequence
        const float inv = 1.0f / qscale;
        for (int i = tid; i < 768; i += PIL_THREADS) {
            const int c = i >> 8, uv = i & 255;
            const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
            float v = (float)uv / 255.0f;
            v = v - mean;
            v = v / sd;
            float r = rintf(inv * v);
            r = fminf(fmaxf(r, -128.f), 127.f);
            lut[i] = (signed char)(int)r;
        }
    }

    const int r0 = band * PIL_BAND, r1 = min(crop, r0 + PIL_BAND);
    const bool htable = ah.ksize <= PIL_HTAB_INTS;
    const bool tiled = av.ksize <= PIL_TILE_ROWS && htable;
    const int NH = htable ? (int)ah.ksize : 0, NV = tiled ? (int)av.ksize : 0;
    const int CW = min(min(crop, PIL_CHUNK_COLS), htable ? PIL_HTAB_INTS / NH : PIL_CHUNK_COLS);

    if (tiled && tid < r1 - r0) {
        const PilTap t = pil_build(av, top + r0 + tid, vk + tid * NV);
        vx[tid] = t.xmin;
        vn[tid] = t.n;
    }
    for (int c0 = 0; c0 < crop; c0 += CW) {
        const int cw = min(CW, crop - c0), rb = cw * 3;
        __syncthreads();                                   // the previous chunk's readers are done
        if (tid < cw) {
            PilTap t;
            if (htable) t = pil_build(ah, left + c0 + tid, htab + tid * NH);
            else { t = pil_tap(ah, left + c0 + tid); hww[tid] = pil_weight_sum(ah, t); }
            hx[tid] = t.xmin;
            hn[tid] = t.n;
        }
        __syncthreads();
        if (tiled) {
            for (int s = r0; s < r1;) {
                const int y0 = vx[s - r0];
                int e = s + 1;                             // the most rows whose taps reach at most PIL_TILE_ROWS input rows
                while (e < r1 && vx[e - r0] + vn[e - r0] - y0 <= PIL_TILE_ROWS) ++e;
                const int ny = vx[e - 1 - r0] + vn[e - 1 - r0] - y0;
                // horizontal, in groups of the input rows that fit `raw`: the bytes of a row the chunk's taps reach (the taps'
                // first and last columns ascend with the column), one row per wave, then one column of one row per thread
                const int xs = hx[0], segb = (hx[cw - 1] + hn[cw - 1] - xs) * 3, G = PIL_RAW_BYTES / segb;
                for (int g0 = 0; g0 < ny; g0 += G) {
                    const int gn = min(G, ny - g0);
                    for (int yy = tid >> 6; yy < gn; yy += PIL_THREADS / 64) {
                        const unsigned char *src = img + ((long long)(y0 + g0 + yy) * W + xs) * 3;
                        unsigned char *dst = raw + yy * segb;
#pragma unroll 4
                        for (int o = tid & 63; o < segb; o += 64) dst[o] = src[o];
                    }
                    __syncthreads();
                    for (int it = tid; it < gn * cw; it += PIL_THREADS) {
                        const int yy = it / cw, c = it - yy * cw;
                        const int n = hn[c];
                        const int *k = htab + c * NH;
                        const unsigned char *p = raw + yy * segb + (hx[c] - xs) * 3;
                        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
                        for (int j = 0; j < n; ++j) {
                            const int kj = k[j];
                            a0 += (int)p[3 * j] * kj;
                            a1 += (int)p[3 * j + 1] * kj;
                            a2 += (int)p[3 * j + 2] * kj;
                        }
                        unsigned char *t = tile + (g0 + yy) * rb + c * 3;
                        t[0] = (unsigned char)pil_clip8(a0);
                        t[1] = (unsigned char)pil_clip8(a1);
                        t[2] = (unsigned char)pil_clip8(a2);
                    }
                    __syncthreads();                       // raw is free again; after the last group: the tile is complete
                }
                for (int it = tid; it < (e - s) * rb; it += PIL_THREADS) {         // vertical: one output byte
                    const int rr = it / rb, q = it - rr * rb;
                    int c, ch;
                    if (NCHW) { ch = q / cw; c = q - ch * cw; }                     // consecutive lanes, consecutive output bytes
                    else { c = q / 3; ch = q - c * 3; }
                    const int r = s - r0 + rr, n = vn[r];
                    const int *k = vk + r * NV;
                    const unsigned char *t = tile + (vx[r] - y0) * rb + c * 3 + ch;
                    int a = 1 << 21;
                    for (int j = 0; j < n; ++j) a += (int)t[j * rb] * k[j];
                    pil_store<NCHW>(out, lut, b, crop, s + rr, c0 + c, ch, pil_clip8(a));
                }
                __syncthreads();
                s = e;
            }
        } else {
            const bool active = tid < cw;
            const int SB = min(PIL_BAND, (PIL_TILE_BYTES / 4) / rb);        // output rows whose accumulators fit
            for (int s = r0; s < r1; s += SB) {
                const int ns = min(r1, s + SB) - s;
                __syncthreads();                           // the previous sub-band's readers of vx, vn, vww are done
                if (tid < ns) {
                    const PilTap t = pil_tap(av, top + s + tid);
                    vx[tid] = t.xmin;
                    vn[tid] = t.n;
                    vww[tid] = av.same ? 0.0 : pil_weight_sum(av, t);
                }
                __syncthreads();
                if (active)
                    for (int i = 0; i < ns * 3; ++i) acc[i * cw + tid] = 1 << 21;   // [row][channel][column]: a thread's own entries
                const int y0 = vx[0], y1 = vx[ns - 1] + vn[ns - 1];
                PilTap th;
                double hw = 0.0;
                if (active) {
                    th.xmin = hx[tid];
                    th.n = hn[tid];
                    th.center = ((double)(left + c0 + tid) + 0.5) * ah.scale;
                    if (!htable) hw = hww[tid];
                }
                for (int y = y0; y < y1; ++y) {
                    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
                    if (active) {
                        const unsigned char *p = img + ((long long)y * W + th.xmin) * 3;
                        for (int j = 0; j < th.n; ++j) {
                            const int kj = htable ? htab[tid * NH + j] : pil_coeff(ah, th, hw, j);
                            a0 += (int)p[3 * j] * kj;
                            a1 += (int)p[3 * j + 1] * kj;
                            a2 += (int)p[3 * j + 2] * kj;
                        }
                    }
                    const int h0 = pil_clip8(a0), h1 = pil_clip8(a1), h2 = pil_clip8(a2);
                    for (int rr = 0; rr < ns; ++rr) {      // the output rows whose taps cover input row y (uniform)
                        PilTap tv;
                        tv.xmin = vx[rr];
                        tv.n = vn[rr];
                        const int j = y - tv.xmin;
                        if (j < 0 || j >= tv.n) continue;
                        tv.center = ((double)(top + s + rr) + 0.5) * av.scale;
                        const int kv = pil_coeff(av, tv, vww[rr], j);
                        if (active) {
                            acc[(rr * 3 + 0) * cw + tid] += h0 * kv;
                            acc[(rr * 3 + 1) * cw + tid] += h1 * kv;
                            acc[(rr * 3 + 2) * cw + tid] += h2 * kv;
                        }
                    }
                }
                if (active)
                    for (int i = 0; i < ns * 3; ++i)
                        pil_store<NCHW>(out, lut, b, crop, s + i / 3, c0 + tid, i % 3, pil_clip8(acc[i * cw + tid]));
            }
        }
    }
}
