// ivit_jpeg.h — the device half of include/ivit_jpeg.h: from the quantised coefficients of B files (csrc/ivit_jpeg_host.h decodes them)
// to uint8 HWC pixels, libjpeg's arithmetic with its defaults, bit for bit.  ivit_amd/jpeg.py (reconstruct_reference) is the numpy
// statement.  Two launches over a ragged batch, gridDim.y the file, both reading ONLY the device copy of the descriptor table.
//
// jpeg_idct_kernel.  A workgroup of 256 threads takes 32 consecutive blocks of one file (its components' blocks are one sequence, as
// its coefficients are), eight threads a block.  Thread l of a block loads row l (one 16-byte load), dequantises it with the eight
// bytes of the component's table and puts it into LDS ([block][row][column], a row padded to 9 ints so that the column pass and
// the row pass are both free of bank conflicts beyond the two halves of a wave).  Then jidctint.c: the column pass (thread l owns column l,
// in place), descaled by CONST_BITS - PASS1_BITS = 11 with rounding; the row pass (thread l owns row l), descaled by CONST_BITS +
// PASS1_BITS + 3 = 18 with rounding; libjpeg's range limit, range_limit[(x) & 1023] of a table centred on 128, in closed form: the
// 10-bit value sign-extended, + 128, clamped to 0 .. 255 (values beyond +-512 wrap around, as the table does); one 8-byte store of
// the row into the component's plane [bh 8, bw 8].  The eight threads of a block sit in one wave; the barriers are workgroup
// barriers all threads reach.
//
// The multiplies are 24-bit (v_mul_i32_i24, full rate; a 32-bit integer product is quarter rate): every product is a 13-bit
// constant (at most 25172 < 2^15) times a sum of at most four inputs of a pass.  The host enforces (ivit_jpeg_host.h, "THE BOUND")
// that the absolute values of a column of a dequantised block sum to at most 2950: the inputs of the column pass and their sums are
// below 2^12, its outputs below 2950 * 1.39 * 4 < 2^14 + 38, sums of four below 2^17: far inside 24 bits.  Coefficients that break
// the bound (a graph replay over bytes no decoder produced) give other bytes, never another address.
//
// jpeg_color_kernel.  One thread per output pixel (x, y) of the w x h crop.  Luma is its plane's sample.  Chroma, with dw = ceil(w /
// hs) and dh = ceil(h / vs) the subsampled plane's real size (libjpeg's downsampled_width / _height; what lies beyond is block padding
// and is never read):
//   1x1                 the sample;
//   dw <= 2             replication, sample (y / vs, x / 2): libjpeg keeps its fancy forms for planes wider than two samples;
//   2x1 (h2v1 fancy)    i = x / 2: even x -> (3 s[i] + s[i - 1] + 1) >> 2, odd x -> (3 s[i] + s[i + 1] + 2) >> 2; the first and the
//                       last sample of a row (x = 0; x = 2 dw - 1) are copied;
//   2x2 (h2v2 fancy)    j = y / 2, the nearer row j and the farther row j - 1 (even y) or j + 1 (odd y), clamped to 0 .. dh - 1 (the
//                       context rows above the first and below the last row repeat it): t[i] = 3 near[i] + far[i]; even x -> (3
//                       t[i] + t[i - 1] + 8) >> 4, odd x -> (3 t[i] + t[i + 1] + 7) >> 4; at x = 0 (4 t[0] + 8) >> 4 and at x = 2 dw
//                       - 1 (4 t[dw - 1] + 7) >> 4, which is what clamping i - 1 and i + 1 gives.
// Then jdcolor.c with cb, cr centred on 128: r = y + ((91881 cr + 32768) >> 16), g = y + ((-22554 cb - 46802 cr + 32768) >> 16), b
// = y + ((116130 cb + 32768) >> 16), clamped to 0 .. 255.  One component: r = g = b = y.  Three byte stores.
#pragma once
#include "../../include/ivit_jpeg.h"

#define JPEG_THREADS 256
#define JPEG_WG_BLOCKS 32
#define JPEG_LDS_ROW 9
#define JPEG_LDS_BLOCK 72

// jidctint.c's 1-D pass before the descale; every product a 24-bit one (see above)
__device__ __forceinline__ void jpeg_islow8(const int x[8], int o[8]) {
    int z1 = __mul24(x[2] + x[6], 4433);
    const int e2 = z1 + __mul24(x[6], -15137), e3 = z1 + __mul24(x[2], 6270);
    const int e0 = (x[0] + x[4]) * 8192, e1 = (x[0] - x[4]) * 8192;
    const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    int t0 = x[7], t1 = x[5], t2 = x[3], t3 = x[1];
    z1 = t0 + t3;
    int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int z5 = __mul24(z3 + z4, 9633);
    t0 = __mul24(t0, 2446);
    t1 = __mul24(t1, 16819);
    t2 = __mul24(t2, 25172);
    t3 = __mul24(t3, 12299);
    z1 = __mul24(z1, -7373);
    z2 = __mul24(z2, -20995);
    z3 = __mul24(z3, -16069) + z5;
    z4 = __mul24(z4, -3196) + z5;
    t0 += z1 + z3;
    t1 += z2 + z4;
    t2 += z2 + z3;
    t3 += z1 + z4;
    o[0] = t10 + t3; o[7] = t10 - t3; o[1] = t11 + t2; o[6] = t11 - t2;
    o[2] = t12 + t1; o[5] = t12 - t1; o[3] = t13 + t0; o[4] = t13 - t0;
}

// range_limit[(v) & 1023] of libjpeg's table behind the IDCT
__device__ __forceinline__ unsigned jpeg_range_limit(int v) {
    const int s = ((int)((unsigned)v << 22) >> 22) + 128;
    return (unsigned)min(max(s, 0), 255);
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_idct_kernel(const short *__restrict__ coefs, const ivit_jpeg_desc *__restrict__ desc,
                                                                 unsigned char *__restrict__ workspace) {
    __shared__ int ws[JPEG_WG_BLOCKS * JPEG_LDS_BLOCK];
    const ivit_jpeg_desc *d = desc + blockIdx.y;
    const int n0 = d->bw[0] * d->bh[0], n1 = d->ncomp == 3 ? d->bw[1] * d->bh[1] : 0, n2 = d->ncomp == 3 ? d->bw[2] * d->bh[2] : 0;
    const long long total = (long long)n0 + n1 + n2, first = (long long)blockIdx.x * JPEG_WG_BLOCKS;
    if (first >= total) return;                               // the whole workgroup: the grid is sized for the largest file
    const int blk = threadIdx.x >> 3, l = threadIdx.x & 7;
    const long long g = first + blk;
    const bool active = g < total;
    int *w = ws + blk * JPEG_LDS_BLOCK;
    int comp = 0;
    long long inner = g;
    if (active) {
        if (g >= (long long)n0 + n1) { comp = 2; inner = g - n0 - n1; }
        else if (g >= n0) { comp = 1; inner = g - n0; }
        const int4 raw = *reinterpret_cast<const int4 *>(coefs + d->coef_offset + g * 64 + l * 8);
        const uint2 q = *reinterpret_cast<const uint2 *>(d->qt + comp * 64 + l * 8);
        int *row = w + l * JPEG_LDS_ROW;
        row[0] = (int)(short)(raw.x & 0xFFFF) * (int)(q.x & 255);
        row[1] = (raw.x >> 16) * (int)((q.x >> 8) & 255);
        row[2] = (int)(short)(raw.y & 0xFFFF) * (int)((q.x >> 16) & 255);
        row[3] = (raw.y >> 16) * (int)(q.x >> 24);
        row[4] = (int)(short)(raw.z & 0xFFFF) * (int)(q.y & 255);
        row[5] = (raw.z >> 16) * (int)((q.y >> 8) & 255);
        row[6] = (int)(short)(raw.w & 0xFFFF) * (int)((q.y >> 16) & 255);
        row[7] = (raw.w >> 16) * (int)(q.y >> 24);
    }
    __syncthreads();
    int x[8], o[8];
    if (active) {
#pragma unroll
        for (int r = 0; r < 8; ++r) x[r] = w[r * JPEG_LDS_ROW + l];
        jpeg_islow8(x, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) w[r * JPEG_LDS_ROW + l] = (o[r] + (1 << 10)) >> 11;
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int c = 0; c < 8; ++c) x[c] = w[l * JPEG_LDS_ROW + c];
        jpeg_islow8(x, o);
        unsigned b[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) b[c] = jpeg_range_limit((o[c] + (1 << 17)) >> 18);
        const int bw = d->bw[comp];
        const long long by = inner / bw, bx = inner - by * bw;
        const long long base = d->plane_offset + (comp >= 1 ? (long long)n0 * 64 : 0) + (comp == 2 ? (long long)n1 * 64 : 0);
        uint2 out;
        out.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        out.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
        *reinterpret_cast<uint2 *>(workspace + base + ((by * 8 + l) * bw + bx) * 8) = out;
    }
}

// the chroma sample of pixel (x, y): `p` the component's plane, `pw` its row pitch, dw x dh its real size
__device__ __forceinline__ int jpeg_chroma(const unsigned char *__restrict__ p, int pw, int hs, int vs, int dw, int dh, int x, int y) {
    if (hs == 1) return p[(long long)y * pw + x];
    const int i = x >> 1;
    if (dw <= 2) return p[(long long)(vs == 2 ? y >> 1 : y) * pw + i];
    const int il = max(i - 1, 0), ir = min(i + 1, dw - 1), io = (x & 1) ? ir : il;
    if (vs == 1) {
        const unsigned char *row = p + (long long)y * pw;
        if (io == i) return row[i];                            // the first and the last sample of the row
        return (3 * row[i] + row[io] + 1 + (x & 1)) >> 2;
    }
    const int j = y >> 1, jf = (y & 1) ? min(j + 1, dh - 1) : max(j - 1, 0);
    const unsigned char *near = p + (long long)j * pw, *far = p + (long long)jf * pw;
    const int t = 3 * near[i] + far[i], u = 3 * near[io] + far[io];
    return (3 * t + u + 8 - (x & 1)) >> 4;
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_color_kernel(const unsigned char *__restrict__ workspace,
                                                                  const ivit_jpeg_desc *__restrict__ desc, unsigned char *__restrict__ pixels) {
    const ivit_jpeg_desc *d = desc + blockIdx.y;
    const int w = d->w, h = d->h;
    const long long p = (long long)blockIdx.x * JPEG_THREADS + threadIdx.x;
    if (p >= (long long)w * h) return;
    const int y = (int)(p / w), x = (int)(p - (long long)y * w);
    const unsigned char *p0 = workspace + d->plane_offset;
    const int pw0 = d->bw[0] * 8;
    const int Y = p0[(long long)y * pw0 + x];
    int r = Y, g = Y, b = Y;
    if (d->ncomp == 3) {
        const int hs = d->hs, vs = d->vs, dw = (w + hs - 1) / hs, dh = (h + vs - 1) / vs, pw1 = d->bw[1] * 8;
        const unsigned char *p1 = p0 + (long long)d->bw[0] * d->bh[0] * 64, *p2 = p1 + (long long)d->bw[1] * d->bh[1] * 64;
        const int cb = jpeg_chroma(p1, pw1, hs, vs, dw, dh, x, y) - 128, cr = jpeg_chroma(p2, pw1, hs, vs, dw, dh, x, y) - 128;
        r = Y + ((91881 * cr + 32768) >> 16);
        g = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
        b = Y + ((116130 * cb + 32768) >> 16);
        r = min(max(r, 0), 255);
        g = min(max(g, 0), 255);
        b = min(max(b, 0), 255);
    }
    unsigned char *out = pixels + d->pixel_offset + p * 3;
    out[0] = (unsigned char)r;
    out[1] = (unsigned char)g;
    out[2] = (unsigned char)b;
}
