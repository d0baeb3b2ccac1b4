// ivit_views.h — image views (include/ivit_views.h): a box of an image of a ragged batch, resized as PIL resizes a stand-alone image,
// a crop x crop window of that, optionally mirrored — V views of any images in ONE launch — and the integer sum of the int32 logits
// of the views of one image.
//
// pil_view_kernel.  PIL's im.crop(box).resize((rw, rh), BICUBIC) resamples the box as an image of its own: the taps clamp at the
// box's edges.  That is the arithmetic ivit_preprocess.h states (its pil_* helpers are used as they are), on a sub-image whose row
// stride is the image's: the source starts at pixels + offset + (y0 w + x0) 3, a row is w pixels further on, the axes are
// pil_axis(bw, rw) and pil_axis(bh, rh), and left / top come from the descriptor instead of the centre-crop rule.  The work shape is
// pil_eval_kernel's, word for word: ceil(crop / PIL_BAND) x V workgroups, the form (tiled or streaming) chosen per view from (bh, rh)
// alone — and, like the horizontal table, from (bw, rw) —, the same tap tables and `raw` staging, the same LDS layout.  A mirrored
// view differs in the store alone (column crop - 1 - col: pil_view_store), chosen per workgroup.  Every tap index lies in [0, bw) x
// [0, bh): a view reads no byte outside its box, and the host checks of the launcher put every box inside its image.
//
// Why pil_view_body repeats pil_eval_kernel's loops instead of both kernels sharing one __device__ body: the shared form was built
// and measured (tools/views_bench.py against the parent's library, interleaved on one box).  It computed the same bytes, but
// ivit_eval_transform_u8 came out 1 % slower (366.9 against 363.4 us at 256 images of 500 x 375; 516.4 against 511.1 us ragged: the
// same instructions under another register allocation) where the parent differs from itself by 0.2 us, so pil_eval_kernel stays as
// it was and this kernel has a body of its own (profiles/README.md, "Image views").  A change to one body belongs in the other.
//
// logits_view_sum_kernel.  [groups views, C] int32 -> [groups, C] int32, row g the sum of rows g views .. g views + views - 1 in int64,
// saturated to int32.  A plain stream, 64-bit indices: VEC takes four classes per thread through 16-byte accesses (C a multiple of 4
// and both pointers 16-byte aligned: then every row is), the other form one class per thread.
#pragma once
#include "ivit_preprocess.h"
#include "../../include/ivit_views.h"

// FLIP: the store goes to column crop - 1 - col, PIL's transpose(FLIP_LEFT_RIGHT) of the crop
template <bool NCHW, bool FLIP>
__device__ __forceinline__ void pil_view_store(unsigned char *__restrict__ out, const signed char *lut, int b, int crop, int row, int col,
                                               int ch, int v) {
    if (FLIP) col = crop - 1 - col;
    if (NCHW) out[(((long long)b * 3 + ch) * crop + row) * crop + col] = (unsigned char)lut[ch * 256 + v];
    else out[(((long long)b * crop + row) * crop + col) * 3 + ch] = (unsigned char)v;
}

// What a view is cut from: `img` the first byte of the box, `W` the pixels from one of its rows to the next (the whole image's
// width), the two axes (input length: the box's side, output length: the resized side), the window's corner in the resized box.
struct PilGeom {
    const unsigned char *img;
    int W;
    PilAxis ah, av;
    long long left, top;
};

// view b, band `band` of it: all of a workgroup's work
template <bool NCHW, bool FLIP>
__device__ __forceinline__ void pil_view_body(const PilGeom &geo, int b, int band, int crop, float m0, float m1, float m2, float s0,
                                              float s1, float s2, float qscale, unsigned char *__restrict__ out) {
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
    const unsigned char *img = geo.img;
    const int W = geo.W;
    const long long top = geo.top, left = geo.left;
    const PilAxis ah = geo.ah, av = geo.av;

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
                    pil_view_store<NCHW, FLIP>(out, lut, b, crop, s + rr, c0 + c, ch, pil_clip8(a));
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
                        pil_view_store<NCHW, FLIP>(out, lut, b, crop, s + i / 3, c0 + tid, i % 3, pil_clip8(acc[i * cw + tid]));
            }
        }
    }
}

template <bool NCHW>
__global__ __launch_bounds__(PIL_THREADS) void pil_view_kernel(const unsigned char *__restrict__ pixels,
                                                               const ivit_image_desc *__restrict__ desc,
                                                               const ivit_view_desc *__restrict__ views, int crop, int nbands, float m0,
                                                               float m1, float m2, float s0, float s1, float s2, float qscale,
                                                               unsigned char *__restrict__ out) {
    const int v = blockIdx.x / nbands, band = blockIdx.x - v * nbands;
    const ivit_view_desc vd = views[v];
    const ivit_image_desc d = desc[vd.image];
    PilGeom geo;
    geo.img = pixels + d.offset + ((long long)vd.y0 * d.w + vd.x0) * 3;
    geo.W = d.w;
    geo.top = vd.top;
    geo.left = vd.left;
    geo.ah = pil_axis(vd.bw, vd.rw);
    geo.av = pil_axis(vd.bh, vd.rh);
    if (vd.flip) pil_view_body<NCHW, true>(geo, v, band, crop, m0, m1, m2, s0, s1, s2, qscale, out);
    else pil_view_body<NCHW, false>(geo, v, band, crop, m0, m1, m2, s0, s1, s2, qscale, out);
}

#define VIEW_SUM_THREADS 256
#define VIEW_SUM_MAX_VIEWS 64

__device__ __forceinline__ int view_sum_sat(long long s) {
    return (int)(s < -2147483648ll ? -2147483648ll : (s > 2147483647ll ? 2147483647ll : s));
}

// n: outputs (VEC: groups of four outputs) in all; per: outputs (groups of four) in a row
template <bool VEC>
__global__ __launch_bounds__(VIEW_SUM_THREADS) void logits_view_sum_kernel(const int *__restrict__ logits, long long n, long long per,
                                                                           int views, int *__restrict__ out) {
    const long long step = (long long)gridDim.x * VIEW_SUM_THREADS;
    for (long long i = (long long)blockIdx.x * VIEW_SUM_THREADS + threadIdx.x; i < n; i += step) {
        const long long g = i / per, c = i - g * per;
        const long long first = g * views * per + c;                     // row g views, the same column
        if (VEC) {
            const int4 *src = reinterpret_cast<const int4 *>(logits);
            long long a0 = 0, a1 = 0, a2 = 0, a3 = 0;
            for (int v = 0; v < views; ++v) {
                const int4 x = src[first + v * per];
                a0 += x.x;
                a1 += x.y;
                a2 += x.z;
                a3 += x.w;
            }
            reinterpret_cast<int4 *>(out)[i] = make_int4(view_sum_sat(a0), view_sum_sat(a1), view_sum_sat(a2), view_sum_sat(a3));
        } else {
            long long a = 0;
            for (int v = 0; v < views; ++v) a += logits[first + v * per];
            out[i] = view_sum_sat(a);
        }
    }
}
