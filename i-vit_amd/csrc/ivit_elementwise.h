// ivit_elementwise.h — wavefront-reduction + shift kernels for gfx950:
// I-LayerNorm(+requant), Shiftmax, ShiftGELU(+requant), dyadic requant, patch
// gather, embedding finish, input quantisation.  All are HBM-bound streaming
// kernels: 16-byte coalesced loads/stores, rows staged in LDS where the torch
// summation order needs strided re-reads.
#pragma once
#include "ivit_device.h"

// ---------------------------------------------------------------------------
// a4: input quantisation (quant_utils.py:12-48,77-96)
__global__ __launch_bounds__(256) void quantize_input_kernel(const float *__restrict__ x, float scale,
                                                             int8_t *__restrict__ q, long long n) {
    const float inv = 1.0f / scale;
    long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    const long long stride = (long long)gridDim.x * 256 * 4;
    for (; i < n; i += stride) {
        if (i + 4 <= n) {
            v4f v = *reinterpret_cast<const v4f *>(x + i);
            unsigned pack = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float r = rintf(inv * v[e]);
                r = fminf(fmaxf(r, -128.f), 127.f);
                pack |= ((unsigned)((int)r) & 0xffu) << (8 * e);
            }
            *reinterpret_cast<unsigned *>(q + i) = pack;
        } else {
            for (long long j = i; j < n; ++j) {
                float r = rintf(inv * x[j]);
                r = fminf(fmaxf(r, -128.f), 127.f);
                q[j] = (int8_t)(int)r;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// N3 (part): ToTensor -> Normalize -> input QuantAct on the device (utils/data_utils.py:89-91, then a4):
//   q = clamp(rne(fl(fl(1/s) * fl(fl(fl(u / 255) - mean[c]) / std[c]))), -128, 127)   for a uint8 pixel u.
// Only 3 x 256 distinct inputs exist: every block rebuilds that table with the exact fp32 sequence (IEEE
// divisions, -ffp-contract=off) and the image pass is a byte gather with the HWC -> CHW transpose.
__global__ __launch_bounds__(256) void normalize_quantize_u8_kernel(const unsigned char *__restrict__ u, int B, int H, int W,
                                                                    float m0, float m1, float m2, float s0, float s1,
                                                                    float s2, float scale, int8_t *__restrict__ q) {
    __shared__ signed char lut[3][256];
    const int tid = threadIdx.x;
    const float inv = 1.0f / scale;
    for (int i = tid; i < 768; i += 256) {
        const int c = i >> 8, uv = i & 255;
        const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
        float v = (float)uv / 255.0f;
        v = v - mean;
        v = v / sd;
        float r = rintf(inv * v);
        r = fminf(fmaxf(r, -128.f), 127.f);
        lut[c][uv] = (signed char)(int)r;
    }
    __syncthreads();
    const long long HW = (long long)H * W, total = (long long)B * HW;      // one thread per pixel (3 bytes in, 3 out)
    for (long long i = (long long)blockIdx.x * 256 + tid; i < total; i += (long long)gridDim.x * 256) {
        const long long b = i / HW, p = i - b * HW;
        const unsigned char *src = u + i * 3;
        int8_t *dst = q + b * 3 * HW + p;
        dst[0] = lut[0][src[0]];
        dst[HW] = lut[1][src[1]];
        dst[2 * HW] = lut[2][src[2]];
    }
}

// ---------------------------------------------------------------------------
// N3: Resize(size, bicubic) + CenterCrop(crop) of the reference's eval transform (utils/data_utils.py:82-88) on
// the device, uint8 HWC in / uint8 HWC out.  The reference resizes with PIL (absent from this image: no pin
// possible); the algorithm restated here is the antialiased separable bicubic (a = -0.5, support scaled by the
// down-scale factor, weights normalised per output pixel) as torch's F.interpolate(mode="bicubic", antialias=True)
// defines it, in fp32 with this fixed operation order (oracle/oracle.py::resize_center_crop_u8 restates it line by
// line; tests/golden/resize.npz pins the oracle against torch within 1 LSB on < 1e-3 of the pixels).
// Two passes: horizontal into an fp32 workspace (only the cropped columns), then vertical + rne + clamp.
__device__ __forceinline__ float cubic_aa(float x) {
    const float a = -0.5f;
    x = fabsf(x);
    if (x < 1.0f) return ((a + 2.0f) * x - (a + 3.0f)) * x * x + 1.0f;
    if (x < 2.0f) return (((a * x) - (5.0f * a)) * x + (8.0f * a)) * x - (4.0f * a);
    return 0.0f;
}
// taps of output index i along one axis: first input index and count; the weights are re-evaluated by `tap_w`
struct AaTaps { int xmin, xsize; float center, invscale, total; };
__device__ __forceinline__ AaTaps aa_taps(int i, int in_size, int out_size) {
    AaTaps t;
    const float scale = (float)in_size / (float)out_size;
    const float support = scale >= 1.0f ? 2.0f * scale : 2.0f;
    t.invscale = scale >= 1.0f ? 1.0f / scale : 1.0f;
    t.center = scale * ((float)i + 0.5f);
    t.xmin = max((int)(t.center - support + 0.5f), 0);
    t.xsize = min((int)(t.center + support + 0.5f), in_size) - t.xmin;
    float tot = 0.0f;
    for (int j = 0; j < t.xsize; ++j) tot += cubic_aa(((float)(j + t.xmin) - t.center + 0.5f) * t.invscale);
    t.total = tot;
    return t;
}
__device__ __forceinline__ float tap_w(const AaTaps &t, int j) {
    return cubic_aa(((float)(j + t.xmin) - t.center + 0.5f) * t.invscale) / t.total;
}
// pass 1: tmp[b, y, xo, c] = sum_j w_j * in[b, y, xmin + j, c] for the cropped output columns xo
__global__ __launch_bounds__(256) void resize_h_kernel(const unsigned char *__restrict__ in, int B, int H0, int W0, int Wr,
                                                       int left, int crop, float *__restrict__ tmp) {
    const long long total = (long long)B * H0 * crop;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int xo = (int)(i % crop);
        const long long by = i / crop;                       // b * H0 + y
        const AaTaps t = aa_taps(xo + left, W0, Wr);
        const unsigned char *row = in + (by * W0 + t.xmin) * 3;
        float w = tap_w(t, 0);
        float a0 = (float)row[0] * w, a1 = (float)row[1] * w, a2 = (float)row[2] * w;
        for (int j = 1; j < t.xsize; ++j) {
            w = tap_w(t, j);
            a0 += (float)row[j * 3] * w;
            a1 += (float)row[j * 3 + 1] * w;
            a2 += (float)row[j * 3 + 2] * w;
        }
        float *o = tmp + i * 3;
        o[0] = a0; o[1] = a1; o[2] = a2;
    }
}
// pass 2: out[b, yo, xo, c] = clamp(rne(sum_j w_j * tmp[b, ymin + j, xo, c]), 0, 255) for the cropped rows yo
__global__ __launch_bounds__(256) void resize_v_kernel(const float *__restrict__ tmp, int B, int H0, int Hr, int top, int crop,
                                                       unsigned char *__restrict__ out) {
    const long long total = (long long)B * crop * crop;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int xo = (int)(i % crop);
        const int yo = (int)((i / crop) % crop);
        const long long b = i / ((long long)crop * crop);
        const AaTaps t = aa_taps(yo + top, H0, Hr);
        const float *col = tmp + ((b * H0 + t.xmin) * crop + xo) * 3;
        const long long rs = (long long)crop * 3;
        float w = tap_w(t, 0);
        float a0 = col[0] * w, a1 = col[1] * w, a2 = col[2] * w;
        for (int j = 1; j < t.xsize; ++j) {
            w = tap_w(t, j);
            a0 += col[j * rs] * w;
            a1 += col[j * rs + 1] * w;
            a2 += col[j * rs + 2] * w;
        }
        unsigned char *o = out + i * 3;
        o[0] = (unsigned char)(int)fminf(fmaxf(rintf(a0), 0.f), 255.f);
        o[1] = (unsigned char)(int)fminf(fmaxf(rintf(a1), 0.f), 255.f);
        o[2] = (unsigned char)(int)fminf(fmaxf(rintf(a2), 0.f), 255.f);
    }
}

// ---------------------------------------------------------------------------
// a3: generic dyadic requant (quant_utils.py:213-253); one thread per element group
template <typename ZT, int BITS>
__global__ __launch_bounds__(256) void requant_kernel(const ZT *__restrict__ z, const ivit_dyadic *__restrict__ dy,
                                                      int nch, const int32_t *__restrict__ z_id,
                                                      const ivit_dyadic *__restrict__ dy_id, void *__restrict__ out,
                                                      long long total, int C) {
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long stride = (long long)gridDim.x * 256;
    ivit_dyadic did = {0.0, 0.0};
    if (z_id) did = dy_id[0];
    for (; i < total; i += stride) {
        int c = (int)(i % C);
        ivit_dyadic d = dy[nch == 1 ? 0 : c];
        double o = rq_f64((double)z[i], d.m, d.r);
        if (z_id) o = rq_f64((double)z_id[i], did.m, did.r) + o;
        int v = clamp_b<BITS>(o);
        if (BITS == 8) reinterpret_cast<int8_t *>(out)[i] = (int8_t)v;
        else if (BITS == 16) reinterpret_cast<int16_t *>(out)[i] = (int16_t)v;
        else reinterpret_cast<int32_t *>(out)[i] = v;
    }
}

// the same for C % 8 == 0: one thread per 8 consecutive channels (one 32-bit index split per thread
// instead of a 64-bit modulo per element)
template <typename ZT, int BITS>
__global__ __launch_bounds__(256) void requant_vec8_kernel(const ZT *__restrict__ z, const ivit_dyadic *__restrict__ dy,
                                                           int nch, const int32_t *__restrict__ z_id,
                                                           const ivit_dyadic *__restrict__ dy_id, void *__restrict__ out,
                                                           long long total8, int C8) {
    double cid = 0.0;
    if (z_id) cid = dy_id[0].m * dy_id[0].r;
    const double c0 = dy[0].m * dy[0].r;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total8; i += (long long)gridDim.x * 256) {
        const int c8 = (int)(i % C8);
        const ZT *zp = z + i * 8;
        int ob[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            double c = c0;
            if (nch != 1) { const ivit_dyadic d = dy[c8 * 8 + e]; c = d.m * d.r; }
            double o = __builtin_rint((double)zp[e] * c);
            if (z_id) o = __builtin_rint((double)z_id[i * 8 + e] * cid) + o;
            ob[e] = clamp_b<BITS>(o);
        }
        if (BITS == 8) {
            unsigned lo = 0, hi = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) { lo |= ((unsigned)ob[e] & 0xffu) << (8 * e); hi |= ((unsigned)ob[4 + e] & 0xffu) << (8 * e); }
            *reinterpret_cast<v2i *>(reinterpret_cast<int8_t *>(out) + i * 8) = v2i{(int)lo, (int)hi};
        } else if (BITS == 16) {
            v8s o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (short)ob[e];
            *reinterpret_cast<v8s *>(reinterpret_cast<int16_t *>(out) + i * 8) = o;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) reinterpret_cast<int32_t *>(out)[i * 8 + e] = ob[e];
        }
    }
}

// ---------------------------------------------------------------------------
// a7 (+a3): I-LayerNorm (quant_modules.py:353-386).  32 lanes per row (two rows per
// wavefront, 8 rows per 256-thread block); the row's fl(fl(Q*s)/s) values are staged
// in LDS as fp32 so the two torch-order sums can stride through them.
// OUT8: fused per-channel requant to int8; else write z as float.
template <bool OUT8>
__global__ __launch_bounds__(256) void layernorm_kernel(const int16_t *__restrict__ x, long long rows, int C,
                                                        long long row_stride, float s,
                                                        const float *__restrict__ bias_int,
                                                        const float *__restrict__ sc,
                                                        const ivit_dyadic *__restrict__ dy,
                                                        void *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char dsmem[];
    const int sub = threadIdx.x & 31;
    const int rslot = threadIdx.x >> 5;            // 0..7
    float *xr = reinterpret_cast<float *>(dsmem) + (size_t)rslot * C;
    const long long row = (long long)blockIdx.x * 8 + rslot;
    if (row >= rows) return;                        // whole 32-lane group exits together
    const int16_t *xp = x + row * row_stride;
    const float Cf = (float)C;
    const RcpC sr = rcp_prepare(s);

    // pass 0: coalesced 16-byte loads -> fl(fl(Q*s)/s) -> LDS
    const int nch8 = C >> 3;
    for (int c = sub; c < nch8; c += 32) {
        v8s q = *reinterpret_cast<const v8s *>(xp + c * 8);
        v4f lo, hi;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            lo[e] = requotient_c((float)q[e], sr);
            hi[e] = requotient_c((float)q[4 + e], sr);
        }
        *reinterpret_cast<v4f *>(xr + c * 8) = lo;
        *reinterpret_cast<v4f *>(xr + c * 8 + 4) = hi;
    }
    for (int k = nch8 * 8 + sub; k < C; k += 32) xr[k] = requotient_c((float)xp[k], sr);
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

    float sum = torch_order_sum32(C, sub, [&](int idx) { return xr[idx]; });
    const float mean = rintf(sum / Cf);
    float var = torch_order_sum32(C, sub, [&](int idx) {
        float y = xr[idx] - mean;
        return y * y;
    });
    float k = 65536.0f;
#pragma unroll
    for (int it = 0; it < 10; ++it) k = floorf((k + floorf(var / k)) * 0.5f);
    const float F = floorf((1.0f / k) * 2147483648.0f);

    // output pass: 8 consecutive channels per lane
    for (int c = sub; c < nch8; c += 32) {
        v4f a = *reinterpret_cast<const v4f *>(xr + c * 8);
        v4f b = *reinterpret_cast<const v4f *>(xr + c * 8 + 4);
        v4f bi0 = *reinterpret_cast<const v4f *>(bias_int + c * 8);
        v4f bi1 = *reinterpret_cast<const v4f *>(bias_int + c * 8 + 4);
        v4f sc0 = *reinterpret_cast<const v4f *>(sc + c * 8);
        v4f sc1 = *reinterpret_cast<const v4f *>(sc + c * 8 + 4);
        float zz[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float xv = e < 4 ? a[e] : b[e - 4];
            float bi = e < 4 ? bi0[e] : bi1[e - 4];
            float scv = e < 4 ? sc0[e] : sc1[e - 4];
            float y = xv - mean;
            float yi = floorf((y * F) * 0.5f);
            float o = yi + bi;
            float Xo = o * scv;
            zz[e] = rintf(lean_div(Xo, rcp_prepare(scv)));
        }
        if (OUT8) {
            unsigned pk[2] = {0, 0};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                ivit_dyadic d = dy[c * 8 + e];
                int v = rq_c((double)zz[e], d.m * d.r, -128, 127);
                pk[e >> 2] |= ((unsigned)v & 0xffu) << (8 * (e & 3));
            }
            *reinterpret_cast<v2i *>(reinterpret_cast<int8_t *>(out) + row * C + c * 8) = v2i{(int)pk[0], (int)pk[1]};
        } else {
            float *zo = reinterpret_cast<float *>(out) + row * C + c * 8;
            *reinterpret_cast<v4f *>(zo) = v4f{zz[0], zz[1], zz[2], zz[3]};
            *reinterpret_cast<v4f *>(zo + 4) = v4f{zz[4], zz[5], zz[6], zz[7]};
        }
    }
    for (int kx = nch8 * 8 + sub; kx < C; kx += 32) {
        float y = xr[kx] - mean;
        float yi = floorf((y * F) * 0.5f);
        float o = yi + bias_int[kx];
        float Xo = o * sc[kx];
        float zv = rintf(Xo / sc[kx]);
        if (OUT8) {
            ivit_dyadic d = dy[kx];
            reinterpret_cast<int8_t *>(out)[row * C + kx] = (int8_t)clamp_b<8>(rq_f64((double)zv, d.m, d.r));
        } else {
            reinterpret_cast<float *>(out)[row * C + kx] = zv;
        }
    }
}

// ---------------------------------------------------------------------------
// a7 + a3, production form.  16 lanes per row (4 rows per wavefront, 16 per 256-thread block,
// LN_RITER row groups per block): per-channel constants — sc, its refined reciprocal, bias_int
// and the requant multiplier c = m*2^-e — are staged once per block in LDS; the integer Newton
// iteration leaves its loop as soon as every row of the wavefront sits on a fixed point
// (k' == k implies all later iterates equal k, so the early exit is exact).
#define LN_RITER 4
template <int CC>   // CC: channel count when known at compile time (loops unroll, no bound tests), 0 = run-time
__global__ __launch_bounds__(256) void layernorm16_kernel(const int16_t *__restrict__ x, long long rows, int C_rt,
                                                          long long row_stride, float s,
                                                          const float *__restrict__ bias_int,
                                                          const float *__restrict__ sc,
                                                          const ivit_dyadic *__restrict__ dy,
                                                          int8_t *__restrict__ out, int riter) {
    const int C = CC ? CC : C_rt;
    extern __shared__ __attribute__((aligned(16))) char dsmem[];
    const int LD = C + 16;                                   // row stride (floats): skews rows by 16 banks
    float *xrows = reinterpret_cast<float *>(dsmem);          // [16][LD]
    double *cC = reinterpret_cast<double *>(dsmem + (size_t)16 * LD * 4);   // [C]
    float *cSc = reinterpret_cast<float *>(cC + C);            // [C]
    float *cY = cSc + C;                                       // [C]
    float *cB = cY + C;                                        // [C]
    const int tid = threadIdx.x;
    for (int c = tid; c < C; c += 256) {
        const float scv = sc[c];
        cSc[c] = scv;
        cY[c] = rcp_prepare(scv).y;
        cB[c] = bias_int[c];
        cC[(c & 7) * (C >> 3) + (c >> 3)] = dy[c].m * dy[c].r;   // [e][chunk]: a lane group reads consecutive doubles
    }
    __syncthreads();
    const int sub = tid & 15, slot = tid >> 4;
    float *xr = xrows + (size_t)slot * LD;
    const RcpC sr = rcp_prepare(s);
    const float Cf = (float)C;
    const int nch8 = C >> 3;
    for (int it = 0; it < riter; ++it) {       // riter row groups per block: chosen by the host to fill the chip
        const long long row_raw = ((long long)blockIdx.x * riter + it) * 16 + slot;
        const bool live = row_raw < rows;
        const long long row = live ? row_raw : rows - 1;     // dead groups recompute the last row, store nothing
        const int16_t *xp = x + row * row_stride;
        for (int c = sub; c < nch8; c += 16) {
            v8s q = *reinterpret_cast<const v8s *>(xp + c * 8);
            v4f lo, hi;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                lo[e] = requotient_c((float)q[e], sr);
                hi[e] = requotient_c((float)q[4 + e], sr);
            }
            const int pc = (c * 8) ^ (((c >> 2) & 3) << 3);   // bank swizzle: rotate 8-float groups by row
            *reinterpret_cast<v4f *>(xr + pc) = lo;
            *reinterpret_cast<v4f *>(xr + pc + 4) = hi;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        auto xat = [&](int idx) { return xr[idx ^ (((idx >> 5) & 3) << 3)]; };
        const float sum = torch_order_sum16(C, sub, xat);
        const float mean = rintf(sum / Cf);
        const float var = torch_order_sum16(C, sub, [&](int idx) {
            float y = xat(idx) - mean;
            return y * y;
        });
        float k = 65536.0f;
        for (int n = 0; n < 10; ++n) {
            const float kn = floorf((k + floorf(var / k)) * 0.5f);
            const bool same = (kn == k);
            k = kn;
            if (__all(same)) break;
        }
        const float F = floorf((1.0f / k) * 2147483648.0f);
        // fl(fl(y * F) * 0.5) == fl(y * (F * 0.5)): a power-of-two factor commutes with the rounding (no subnormals here)
        const float Fh = F * 0.5f;
        for (int c = sub; c < nch8; c += 16) {
            const int pc = (c * 8) ^ (((c >> 2) & 3) << 3);
            const v4f a = *reinterpret_cast<const v4f *>(xr + pc), b = *reinterpret_cast<const v4f *>(xr + pc + 4);
            const v4f bi0 = *reinterpret_cast<const v4f *>(cB + c * 8), bi1 = *reinterpret_cast<const v4f *>(cB + c * 8 + 4);
            const v4f sc0 = *reinterpret_cast<const v4f *>(cSc + c * 8), sc1 = *reinterpret_cast<const v4f *>(cSc + c * 8 + 4);
            const v4f y0 = *reinterpret_cast<const v4f *>(cY + c * 8), y1 = *reinterpret_cast<const v4f *>(cY + c * 8 + 4);
            unsigned pk[2] = {0, 0};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xv = e < 4 ? a[e] : b[e - 4];
                const float bi = e < 4 ? bi0[e] : bi1[e - 4];
                RcpC rc;
                rc.d = e < 4 ? sc0[e] : sc1[e - 4];
                rc.y = e < 4 ? y0[e] : y1[e - 4];
                const float y = xv - mean;
                const float yi = floorf(y * Fh);
                const float o = yi + bi;
                const float zz = rintf(lean_div(o * rc.d, rc));
                const int v = rq_c((double)zz, cC[e * nch8 + c], -128, 127);
                pk[e >> 2] |= ((unsigned)v & 0xffu) << (8 * (e & 3));
            }
            if (live) *reinterpret_cast<v2i *>(out + row * C + c * 8) = v2i{(int)pk[0], (int)pk[1]};
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
}

// ---------------------------------------------------------------------------
// a5: Shiftmax (quant_modules.py:469-497).  One wavefront per row; the row's exp
// values are staged in LDS (fp32) for the torch-order sum done by lanes 0..31.
__global__ __launch_bounds__(256) void shiftmax_kernel(const int8_t *__restrict__ x, long long rows, int n,
                                                       int ld_in, float s, int out_bits,
                                                       uint16_t *__restrict__ out, int ld_out) {
    extern __shared__ __attribute__((aligned(16))) char dsmem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *er = reinterpret_cast<float *>(dsmem) + (size_t)wave * n;
    const long long row = (long long)blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const int8_t *xp = x + row * ld_in;
    // row max: fl(fl(Q*s)/s) is monotone in Q (s > 0), so take the integer max first
    int qmax = -128;
    for (int j = lane; j < n; j += 64) qmax = max(qmax, (int)xp[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) qmax = max(qmax, __shfl_xor(qmax, o));
    const RcpC sr = rcp_prepare(s);
    const float mx = requotient_c((float)qmax, sr);
    const float x0 = floorf(-1.0f / s);
    const RcpC x0r = rcp_prepare(x0);
    const float nx0 = 15.0f * x0;
    for (int j = lane; j < n; j += 64) {
        float xt = requotient_c((float)xp[j], sr);
        er[j] = shift_exp_c(xt - mx, x0r, nx0, 15);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    float S = torch_order_sum32(n, lane & 31, [&](int idx) { return er[idx]; });
    const float F = recip_factor(S);
    const float div = ldexpf(1.0f, out_bits - 32);  // 1 / 2**(31-bits+1), exact
    uint16_t *op = out + row * ld_out;
    for (int j = lane; j < n; j += 64) op[j] = (uint16_t)(int)floorf((er[j] * F) * div);
}

// ---------------------------------------------------------------------------
// a6 (+a3): ShiftGELU (quant_modules.py:410-445).  One wavefront per token row.
template <bool OUT8>
__global__ __launch_bounds__(256) void shiftgelu_kernel(const int8_t *__restrict__ x, long long rows, int C, float s,
                                                        ivit_dyadic dy, void *__restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const int8_t *xp = x + row * C;
    const int nch = C >> 4;
    int qmax = -128;
    for (int c = lane; c < nch; c += 64) {
        v4i v = *reinterpret_cast<const v4i *>(xp + c * 16);
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int b = 0; b < 4; ++b) qmax = max(qmax, (int)(int8_t)((unsigned)v[d] >> (8 * b)));
    }
    for (int k = nch * 16 + lane; k < C; k += 64) qmax = max(qmax, (int)xp[k]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) qmax = max(qmax, __shfl_xor(qmax, o));
    const float mx = requotient((float)qmax, s);
    const float ssig = s * 1.702f;
    const float x0 = floorf(-1.0f / ssig);
    const float nx0 = 23.0f * x0;
    const float emax = shift_exp(-mx, x0, nx0, 23);

    auto one = [&](int q) -> int {
        float p = requotient((float)q, s);
        float e = shift_exp(p - mx, x0, nx0, 23);
        float F = recip_factor(e + emax);
        float sig = floorf((e * F) * 5.9604644775390625e-08f);  // / 2**24
        // next QuantAct rounds p*sig back to the integer Q*sig (quant_utils.py:220)
        int prod = (int)rintf(p * sig);
        if (OUT8) return clamp_b<8>(rq_f64((double)prod, dy.m, dy.r));
        return prod;
    };

    for (int c = lane; c < nch; c += 64) {
        v4i v = *reinterpret_cast<const v4i *>(xp + c * 16);
        if (OUT8) {
            v4i o;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                unsigned pk = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    pk |= ((unsigned)one((int)(int8_t)((unsigned)v[d] >> (8 * b))) & 0xffu) << (8 * b);
                o[d] = (int)pk;
            }
            *reinterpret_cast<v4i *>(reinterpret_cast<int8_t *>(out) + row * C + c * 16) = o;
        } else {
            int16_t *op = reinterpret_cast<int16_t *>(out) + row * C + c * 16;
            v4i o0, o1;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                int r0 = one((int)(int8_t)((unsigned)v[d])), r1 = one((int)(int8_t)((unsigned)v[d] >> 8));
                int r2 = one((int)(int8_t)((unsigned)v[d] >> 16)), r3 = one((int)(int8_t)((unsigned)v[d] >> 24));
                int w0 = (r0 & 0xffff) | (r1 << 16), w1 = (r2 & 0xffff) | (r3 << 16);
                if (d < 2) { o0[2 * d] = w0; o0[2 * d + 1] = w1; }
                else { o1[2 * (d - 2)] = w0; o1[2 * (d - 2) + 1] = w1; }
            }
            *reinterpret_cast<v4i *>(op) = o0;
            *reinterpret_cast<v4i *>(op + 8) = o1;
        }
    }
    for (int k = nch * 16 + lane; k < C; k += 64) {
        int r = one((int)xp[k]);
        if (OUT8) reinterpret_cast<int8_t *>(out)[row * C + k] = (int8_t)r;
        else reinterpret_cast<int16_t *>(out)[row * C + k] = (int16_t)r;
    }
}

// ---------------------------------------------------------------------------
// a8: patch gather (layers_quant.py:184-196): NCHW int8 -> [B*gh*gw, Cin*P*P],
// element order (c, py, px) = conv weight order.  One block per (image, patch row): the Cin*P image
// rows of the strip are read as whole contiguous rows into LDS and leave as gw contiguous patch rows —
// both HBM sides fully coalesced (the one-pass form fetched 5x the algorithmic bytes).
__global__ __launch_bounds__(256) void im2col_patch_kernel(const int8_t *__restrict__ img, int B, int Cin, int H,
                                                           int W, int P, int8_t *__restrict__ rows) {
    extern __shared__ __attribute__((aligned(16))) char dsmem[];
    const int gh = H / P, gw = W / P, K = Cin * P * P;
    const int b = blockIdx.x / gh, gy = blockIdx.x - b * gh;
    const int S = Cin * P * W;                       // strip bytes, layout [c][py][x]
    const int tid = threadIdx.x;
    for (int idx = tid * 4; idx < S; idx += 256 * 4) {
        const int x = idx % W, r = idx / W, py = r % P, c = r / P;
        *reinterpret_cast<int *>(dsmem + idx) =
            *reinterpret_cast<const int *>(img + (((long long)b * Cin + c) * H + gy * P + py) * W + x);
    }
    __syncthreads();
    int8_t *dst = rows + ((long long)b * gh + gy) * gw * K;
    for (int o = tid * 4; o < S; o += 256 * 4) {
        const int gx = o / K, kk = o - gx * K;
        const int px = kk % P, r = kk / P;           // r = c*P + py
        *reinterpret_cast<int *>(dst + o) = *reinterpret_cast<const int *>(dsmem + r * W + gx * P + px);
    }
}

// P = 16: a patch row (c, py) is exactly one 16-byte chunk on both sides, so the strip moves as 16-byte chunks with no
// division by a run-time value (the generic kernel above spends ~26 VALU instructions per BYTE on them: 1.6e7
// wave-instructions per launch at batch 256).  Threads are a 16 x 16 grid over (x chunk, strip row) for the load — the
// row's channel advances by one every 16 rows — and walk (patch, row) pairs with a compile-time divisor for the store.
template <int CIN>
__global__ __launch_bounds__(256) void im2col_patch16_kernel(const int8_t *__restrict__ img, int H, int W, int8_t *__restrict__ rows) {
    extern __shared__ __attribute__((aligned(16))) char dsmem[];
    constexpr int P = 16, R = CIN * P, K = CIN * P * P;
    const int gh = H / P, gw = W / P, wc = W / 16;
    const int b = blockIdx.y, gy = blockIdx.x;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int8_t *src = img + ((long long)b * CIN * H + gy * P + ty) * W;      // channel 0, strip row ty
#pragma unroll
    for (int c = 0; c < CIN; ++c)
        for (int xc = tx; xc < wc; xc += 16)
            *reinterpret_cast<v4i *>(dsmem + (c * P + ty) * W + xc * 16) =
                *reinterpret_cast<const v4i *>(src + (long long)c * H * W + xc * 16);
    __syncthreads();
    int8_t *dst = rows + ((long long)b * gh + gy) * gw * K;
    for (int q = tid; q < gw * R; q += 256) {
        const int gx = q / R, r = q - gx * R;                                  // R is a compile-time constant
        *reinterpret_cast<v4i *>(dst + q * 16) = *reinterpret_cast<const v4i *>(dsmem + r * W + gx * 16);
    }
}

// class token + position embedding (vit_quant.py:259-265)
__global__ __launch_bounds__(256) void embed_finish_kernel(const int16_t *__restrict__ patch16,
                                                           const int32_t *__restrict__ z_cls,
                                                           const int16_t *__restrict__ pos, ivit_dyadic dx,
                                                           ivit_dyadic dp, int16_t *__restrict__ x16, int T,
                                                           int D, float inv_d8, int fast, int only_cls = 0) {
    // one thread per 8 channels (16-byte loads/stores), one image per blockIdx.y; (token, channel group) from the flat index
    // by a float reciprocal (exact: T * D / 8 < 2^22), no integer division
    const int D8 = D >> 3, b = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= T * D8) return;
    const int t = (int)(((float)idx + 0.5f) * inv_d8), c8 = idx - t * D8;
    if (only_cls && t != 0) return;        // the patch rows come out of the patch-embedding GEMM's epilogue (ivit_patch_embed)
    const double cx = dx.m * dx.r, cp = dp.m * dp.r;
    const v8s pv = *reinterpret_cast<const v8s *>(pos + (long long)t * D + c8 * 8);
    v8s o;
    if (t == 0) {                      // class token: int32 accumulators, the general requant
        const v4i a0 = *reinterpret_cast<const v4i *>(z_cls + c8 * 8), a1 = *reinterpret_cast<const v4i *>(z_cls + c8 * 8 + 4);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const double v = __builtin_rint((double)pv[e] * cp) + __builtin_rint((double)(e < 4 ? a0[e] : a1[e - 4]) * cx);
            o[e] = (short)clamp_b<16>(v);
        }
    } else {
        const v8s xv = *reinterpret_cast<const v8s *>(patch16 + ((long long)b * (T - 1) + (t - 1)) * D + c8 * 8);
        if (fast) {                    // 16-bit operands, |c| < 2^9: one fma + low dword each (rq_fast), integer sum and clamp
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (short)min(max(rq_fast((int)pv[e], cp) + rq_fast((int)xv[e], cx), -32768), 32767);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const double v = __builtin_rint((double)pv[e] * cp) + __builtin_rint((double)xv[e] * cx);
                o[e] = (short)clamp_b<16>(v);
            }
        }
    }
    *reinterpret_cast<v8s *>(x16 + ((long long)b * T + t) * D + c8 * 8) = o;
}

// ---------------------------------------------------------------------------
// ShiftGELU(+requant) as a table: for a frozen layer (scale s, dyadic dy) the int8
// output is a pure function of (Q, row max), so tab[(qmax+128)*256 + (Q+128)] is
// built ONCE at freeze time by the same faithful device code (64 KB per layer) and
// the per-token work becomes: row max -> copy one 256-byte table row to LDS ->
// byte gathers.  Bit-identical to shiftgelu_kernel<true> by construction
// (tests/test_gpu_parity.py::test_shiftgelu_lut_equals_direct).
__global__ __launch_bounds__(256) void shiftgelu_table_kernel(float s, ivit_dyadic dy, int8_t *__restrict__ tab) {
    const int qmax = (int)blockIdx.x - 128, q = (int)threadIdx.x - 128;
    const float mx = requotient((float)qmax, s);
    const float ssig = s * 1.702f;
    const float x0 = floorf(-1.0f / ssig);
    const float nx0 = 23.0f * x0;
    const float emax = shift_exp(-mx, x0, nx0, 23);
    float p = requotient((float)q, s);
    float e = shift_exp(p - mx, x0, nx0, 23);
    float F = recip_factor(e + emax);
    float sig = floorf((e * F) * 5.9604644775390625e-08f);
    int prod = (int)rintf(p * sig);
    tab[blockIdx.x * 256 + threadIdx.x] = (int8_t)clamp_b<8>(rq_f64((double)prod, dy.m, dy.r));
}

__global__ __launch_bounds__(256) void shiftgelu_lut_kernel(const int8_t *__restrict__ x, long long rows, int C,
                                                            const int8_t *__restrict__ tab,
                                                            int8_t *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) unsigned char lut[4][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const int8_t *xp = x + row * C;
    const int nch = C >> 4;
    int qmax = -128;
    for (int c = lane; c < nch; c += 64) {
        v4i v = *reinterpret_cast<const v4i *>(xp + c * 16);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            // signed byte max of 4 packed int8: compare as sign-extended fields
            int w = v[d];
            qmax = max(qmax, max(max((w << 24) >> 24, (w << 16) >> 24), max((w << 8) >> 24, w >> 24)));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) qmax = max(qmax, __shfl_xor(qmax, o));
    reinterpret_cast<unsigned *>(lut[wave])[lane] =
        reinterpret_cast<const unsigned *>(tab + (qmax + 128) * 256)[lane];
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const unsigned char *L = lut[wave];
    for (int c = lane; c < nch; c += 64) {
        v4i v = *reinterpret_cast<const v4i *>(xp + c * 16);
        v4i o;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            unsigned w = (unsigned)v[d] ^ 0x80808080u;   // Q + 128 per byte
            unsigned r = (unsigned)L[w & 0xff] | ((unsigned)L[(w >> 8) & 0xff] << 8) |
                         ((unsigned)L[(w >> 16) & 0xff] << 16) | ((unsigned)L[w >> 24] << 24);
            o[d] = (int)r;
        }
        *reinterpret_cast<v4i *>(out + row * C + c * 16) = o;
    }
}

// The same, half a wavefront per row and the row held in registers between the two passes (ITER 16-byte chunks per lane:
// C = 512 * ITER ... e.g. 1536 -> 3, 3072 -> 6; narrower rows use the tail mask).  One read of the row instead of two, all
// 64 lanes busy (a 1536-channel row is 96 chunks: 64 + 32 lanes in the one-wave-per-row form), the byte maximum by two
// v_perm + two v_pk_max_u16 per dword on the biased bytes, table addresses as (byte | row's table base).
template <int ITER>
__global__ __launch_bounds__(256) void shiftgelu_lut2_kernel(const int8_t *__restrict__ x, long long rows, int C,
                                                             const int8_t *__restrict__ tab, int8_t *__restrict__ out) {
    __shared__ __attribute__((aligned(256))) unsigned char lut[8][256];
    typedef unsigned short v2us __attribute__((ext_vector_type(2)));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l32 = lane & 31;
    const int slot = wave * 2 + half;
    const long long row_raw = (long long)blockIdx.x * 8 + slot;
    const bool live = row_raw < rows;
    const long long row = live ? row_raw : rows - 1;            // a dead half-wave recomputes the last row, stores nothing
    const int8_t *xp = x + row * C;
    const int nch = C >> 4;
    v4i v[ITER];
    v2us me = {0, 0}, mo = {0, 0};                              // running maxima of the even / odd bytes (biased, unsigned)
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int c = l32 + it * 32;
        v4i t = {(int)0x80808080u, (int)0x80808080u, (int)0x80808080u, (int)0x80808080u};     // -128: neutral for the max
        if (c < nch) t = *reinterpret_cast<const v4i *>(xp + c * 16);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const unsigned w = (unsigned)t[d] ^ 0x80808080u;    // Q + 128 per byte
            t[d] = (int)w;
            me = __builtin_elementwise_max(me, __builtin_bit_cast(v2us, __builtin_amdgcn_perm(0u, w, 0x0c020c00u)));
            mo = __builtin_elementwise_max(mo, __builtin_bit_cast(v2us, __builtin_amdgcn_perm(0u, w, 0x0c030c01u)));
        }
        v[it] = t;
    }
    const v2us m2 = __builtin_elementwise_max(me, mo);
    int qb = max((int)m2[0], (int)m2[1]);                       // biased row maximum of this lane
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) qb = max(qb, __shfl_xor(qb, o));
    // this row's 256-byte table line: lanes 0..31 of the half copy 8 bytes each
    reinterpret_cast<v2i *>(lut[slot])[l32] = reinterpret_cast<const v2i *>(tab + (size_t)qb * 256)[l32];
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const unsigned base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)lut[slot];
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int c = l32 + it * 32;
        v4i o;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const unsigned w = (unsigned)v[it][d];
            const unsigned b0 = *(lds_u8 *)(size_t)(base | (w & 0xffu)), b1 = *(lds_u8 *)(size_t)(base | ((w >> 8) & 0xffu));
            const unsigned b2 = *(lds_u8 *)(size_t)(base | ((w >> 16) & 0xffu)), b3 = *(lds_u8 *)(size_t)(base | (w >> 24));
            o[d] = (int)(b0 | (b1 << 8) | (b2 << 16) | (b3 << 24));
        }
        if (live && c < nch) *reinterpret_cast<v4i *>(out + row * C + c * 16) = o;
    }
}

// diagnostics: lean_div vs the compiler's IEEE division, element-wise
__global__ __launch_bounds__(256) void debug_div_kernel(const float *__restrict__ n, const float *__restrict__ d,
                                                        float *__restrict__ q_ieee, float *__restrict__ q_lean,
                                                        long long count) {
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < count) {
        q_ieee[i] = n[i] / d[i];
        q_lean[i] = lean_div(n[i], rcp_prepare(d[i]));
    }
}
