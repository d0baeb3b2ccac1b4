// ivit_logreg.h — logistic-regression probe (include/ivit_logreg.h): the SUM of the softmax cross-entropy over a batch of labelled int8
// features and its gradient with respect to a float head, in four launches and a workspace.  The [rows, classes] matrix of logits or
// probabilities is never written: the row pass keeps four numbers per row, the gradient pass recomputes the logits it needs.
//
//   z[r, c] = x_scale (W[c, :] . x[r, :]) + b[c]      loss = sum_r logsumexp(z[r, :]) - z[r, label[r]]
//   grad_W  = sum_r (softmax(z[r, :]) - onehot(label[r])) (x) x[r, :]      grad_b = sum_r softmax(z[r, :]) - onehot(label[r])
//   over the rows with 0 <= label < C; every other row counts for nothing.
//
// Operands.  An int8 value is exact in bf16, so the matrix instruction is v_mfma_f32_32x32x16_bf16 and the features convert on the way
//   into it (v_cvt_f32_i32, the high half of the float: no rounding).  A float is the exact sum of LOGREG_PIECES = 3 bf16 numbers
//   (logreg_split3: the leading 8 significant bits, the next 8, the last 8, each by truncation); the product of a piece and an int8
//   value has at most 16 significant bits, so every product is exact and only the fp32 accumulation rounds.  Two pieces would carry 16
//   of a float's 24 bits — a relative 2^-16 on every weight and every probability, three orders above fp32 accumulation at these
//   lengths — so both sides carry three.
// logreg_pieces_kernel  the set-up launch: W fp32 [C, dim] -> its three pieces in the workspace, in the order both passes load them.
//   Block (class tile t of 32, feature pair-step j of 32, piece p) holds, for lane l, the 16 bf16 of class 32 t + l % 32, features
//   32 j + 16 (l / 32) .. + 15: 32 bytes per lane, 2 KB per block, two 16-byte loads per lane.  The first 8 are the lane's operand of
//   k-step 2 j, the second 8 of k-step 2 j + 1 (the order of a contraction is free as long as both operands agree: the feature rows
//   are loaded 16 bytes per lane the same way).  Classes >= C of the last tile are zeros.
// logreg_rows_kernel<KS>  the row statistics, dim = 64 KS: the work shape of kmeans_assign_kernel (ivit_cluster.h).  A workgroup is
//   four wavefronts of 32 rows each; a wavefront keeps its rows as int8 in 8 KS registers for the whole kernel (the B operand, converted
//   per k-step) and walks the class tiles; after 12 KS MFMAs lane l holds, for row l % 32, the logits of classes
//   32 t + (r & 3) + 8 (r >> 2) + 4 (l / 32), r = 0 .. 15, ascending in r.  Within a pair-step the small pieces go first;
//   pair-step j adds into accumulator set j % 4; the sets meet as ((s0 + s1) + s2) + s3.  That is the gradient pass's order
//   (its wavefront w works the pair-steps j = w, w + 4, ... and the four partial sums are added in that order), so both passes hold
//   the SAME BITS of every logit: exp(z - max - log-sum) of a class that dominates its row is then 1 - eps with eps exact, where a
//   logit off by one unit in the last place would put a relative 2^-23 |z| on p - onehot (measured: 1.3e-6 of max|grad| at |z| ~ 10
//   with independent orders, against 3.4e-7 for the fp32 tensor route; profiles/README.md).
//   Per lane, the online-softmax recurrence over its 16 logits of every tile: running maximum,
//   sum of exponentials rescaled when the maximum moves, the label's logit, the first largest logit.  At the end the two lanes of a row
//   exchange their states (cross-lane moves, no LDS) and lane l < 32 writes the row's record {max, log-sum, loss term, flags}
//   (flags: bit 0 the row counts, bit 1 its argmax is its label), 16 bytes.
// logreg_grad_kernel<NT>  the gradient.  Grid (class tiles, parts of the rows); a workgroup owns 32 classes x all of dim and walks its
//   part 32 rows at a time.  Per step: (a) every thread loads 16 features of 4 rows, transposes the 4 x 4 byte blocks in registers
//   (probe_transpose4) and stores them into the [feature][row] image in LDS — 32 bytes per feature, the rows in the order the MFMA's
//   k-slots want them (below), the two 16-byte halves swapped on every second group of 8 features so that a quarter-wave's 16-byte
//   reads meet every bank once; (b) wavefront w recomputes the logits' partial sums over the feature pair-steps j = w, w + 4, ...
//   (A = the rows straight from memory, B = the weight pieces) and leaves them in LDS; (c) every wavefront adds the four partial sums
//   in order and forms g = exp((z - max) - log-sum) - onehot from the rows' records: lane l then holds class l % 32, rows
//   4 (l / 32) + (r & 3) + 8 (r >> 2) — which IS an A operand of the second product if k-slot q of k-step s means row
//   4 (l / 32) + 16 s + (q & 3) + 8 (q >> 2): g goes from accumulator registers into operand registers (split into three pieces) with
//   no transposition, and the image stores the rows in that order; (d) wavefront w owns the feature tiles w, w + 4, ... (NT of them at
//   most): per tile one 16-byte LDS read, six MFMAs into a fresh accumulator, one vector addition into the tile's running sum — one
//   fp32 rounding of the running sum per 32 rows.  grad_b: the lane's sum of g.  A part ends with plain stores of its
//   [32 classes, dim] tile and its 32 bias sums into the workspace.  A part holds at most LOGREG_FLUSH_ROWS rows.
// logreg_reduce_kernel  adds the parts in ascending order into grad_W and grad_b (one thread per element), and its last block adds
//   the rows' loss terms (fp64) and flags (int64): thread t the rows t, t + 256, ... in order, then a fixed tree.
// No atomics anywhere: the same inputs, parts and device give the same bits.  Plain vector stores only, no scratch.
#pragma once
#include "../../include/ivit_logreg.h"
#include "ivit_probe.h"

#define LOGREG_MIN_DIM 64
#define LOGREG_MAX_DIM 1024
#define LOGREG_MAX_CLASSES 65536
#define LOGREG_PIECES 3
#define LOGREG_TILE 32                              // classes of a tile, rows of a step: the M and N of the MFMA
#define LOGREG_RB 128                               // rows of a workgroup of the row pass
#define LOGREG_FLUSH_ROWS 65536                     // rows of a part at most: the length of one fp32 running sum
#define LOGREG_ROW_BYTES 16                         // a row's record in the workspace

typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

struct LogregArgs {
    const int8_t *x;            // [N, dim]
    const int *labels;          // [N]
    const float *W, *b;         // [C, dim], [C]
    v4i *wp;                    // workspace: the weight pieces, [tiles][dim / 32][3][64 lanes] x 32 bytes
    v4f *rowst;                 // workspace: [N] records
    float *pW, *pb;             // workspace: [parts][32 tiles][dim], [parts][32 tiles]
    double *loss;
    float *gW, *gb;
    long long *correct;
    long long N, per;           // part s covers rows [s per, min(N, (s + 1) per)); per is a multiple of 32
    int dim, C, tiles, parts;
    float xs;
};

// the leading 16 bits of three floats that sum to v exactly (every piece 8 significant bits, by truncation)
__device__ __forceinline__ void logreg_split3(float v, unsigned (&o)[3]) {
    o[0] = __float_as_uint(v) >> 16;
    const float r1 = v - __uint_as_float(o[0] << 16);
    o[1] = __float_as_uint(r1) >> 16;
    const float r2 = r1 - __uint_as_float(o[1] << 16);
    o[2] = __float_as_uint(r2) >> 16;
}

// eight int8 (the bytes of d0, then of d1, lowest first) as eight bf16: exact
__device__ __forceinline__ v8bf logreg_bf16x8(int d0, int d1) {
    v4i o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = k < 2 ? d0 : d1;
        const float f0 = (float)(signed char)((unsigned)d >> (16 * (k & 1)));
        const float f1 = (float)(signed char)((unsigned)d >> (16 * (k & 1) + 8));
        o[k] = (int)__builtin_amdgcn_perm(__float_as_uint(f1), __float_as_uint(f0), 0x07060302u);
    }
    return __builtin_bit_cast(v8bf, o);
}

__device__ __forceinline__ v16f logreg_mfma(v4i a, v8bf b, v16f c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, a), b, c, 0, 0, 0);
}
__device__ __forceinline__ v16f logreg_mfma(v8bf a, v4i b, v16f c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(v8bf, b), c, 0, 0, 0);
}
__device__ __forceinline__ v16f logreg_zero16() {
    v16f z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    return z;
}

// one thread per (class tile, pair-step, lane)
__global__ __launch_bounds__(256) void logreg_pieces_kernel(LogregArgs p) {
    const int J = p.dim >> 5;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)p.tiles * J * 64) return;
    const int lane = (int)(t & 63), j = (int)((t >> 6) % J), tile = (int)((t >> 6) / J);
    const int c = tile * LOGREG_TILE + (lane & 31);
    unsigned pc[16][3];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        v4f w = v4f{0.f, 0.f, 0.f, 0.f};
        if (c < p.C) w = *reinterpret_cast<const v4f *>(p.W + (size_t)c * p.dim + 32 * j + 16 * (lane >> 5) + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) logreg_split3(w[e], pc[4 * q + e]);
    }
    v4i *dst = p.wp + ((size_t)(tile * J + j) * LOGREG_PIECES * 64 + lane) * 2;
#pragma unroll
    for (int piece = 0; piece < LOGREG_PIECES; ++piece)
#pragma unroll
        for (int hv = 0; hv < 2; ++hv) {
            v4i o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = (int)(pc[8 * hv + 2 * k][piece] | (pc[8 * hv + 2 * k + 1][piece] << 16));
            dst[(size_t)piece * 128 + hv] = o;
        }
}

template <int KS>
__global__ __launch_bounds__(256) void logreg_rows_kernel(LogregArgs p) {
    constexpr int J = 2 * KS, DIM = 64 * KS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const long long r0 = ((long long)blockIdx.x * 4 + wave) * LOGREG_TILE;
    if (r0 >= p.N) return;                                               // whole wavefronts leave: nothing below synchronises a block
    const long long row = min(r0 + l31, p.N - 1);                        // rows beyond the end: clamped on load, never stored
    v4i xr[J];
    {
        const int8_t *src = p.x + (size_t)row * DIM + 16 * half;
#pragma unroll
        for (int j = 0; j < J; ++j) xr[j] = *reinterpret_cast<const v4i *>(src + 32 * j);
    }
    const int label = p.labels[row];
    const float NEG = -__builtin_inff();
    float m = NEG, s = 0.f, zl = 0.f, bz = NEG;
    int bi = 0x7fffffff, found = 0;
    for (int tile = 0; tile < p.tiles; ++tile) {
        const v4i *w = p.wp + ((size_t)tile * J * LOGREG_PIECES * 64 + lane) * 2;
        v16f acc[4];                                                     // pair-step j adds into set j % 4: the gradient pass's four wavefronts
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = logreg_zero16();
#pragma unroll
        for (int j = 0; j < J; ++j) {
            v4i a[LOGREG_PIECES][2];
#pragma unroll
            for (int piece = 0; piece < LOGREG_PIECES; ++piece) {
                a[piece][0] = w[(size_t)(j * LOGREG_PIECES + piece) * 128];
                a[piece][1] = w[(size_t)(j * LOGREG_PIECES + piece) * 128 + 1];
            }
            const v8bf x0 = logreg_bf16x8(xr[j][0], xr[j][1]), x1 = logreg_bf16x8(xr[j][2], xr[j][3]);
#pragma unroll
            for (int piece = LOGREG_PIECES - 1; piece >= 0; --piece) {   // the small pieces first
                acc[j & 3] = logreg_mfma(a[piece][0], x0, acc[j & 3]);
                acc[j & 3] = logreg_mfma(a[piece][1], x1, acc[j & 3]);
            }
        }
        float z[16], tmax = NEG;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = tile * LOGREG_TILE + (r & 3) + 8 * (r >> 2) + 4 * half;
            const float zs = ((acc[0][r] + acc[1][r]) + acc[2][r]) + acc[3][r];
            z[r] = c < p.C ? p.xs * zs + p.b[c] : NEG;
            tmax = fmaxf(tmax, z[r]);
            if (z[r] > bz) { bz = z[r]; bi = c; }                        // ascending classes: the first of equal logits stays
            if (c == label) { zl = z[r]; found = 1; }
        }
        if (tmax > NEG) {                                                // a lane with no class in this tile keeps its state
            const float mn = fmaxf(m, tmax);
            float e = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) e += expf(z[r] - mn);
            s = s * expf(m - mn) + e;
            m = mn;
        }
    }
    // the two lanes of a row: lane l < 32 holds class 0, so its maximum is finite
    const float om = __shfl_xor(m, 32, 64), os = __shfl_xor(s, 32, 64), ozl = __shfl_xor(zl, 32, 64), obz = __shfl_xor(bz, 32, 64);
    const int obi = __shfl_xor(bi, 32, 64), ofound = __shfl_xor(found, 32, 64);
    if (half == 0 && r0 + l31 < p.N) {
        const float M = fmaxf(m, om), S = s * expf(m - M) + os * expf(om - M), logS = logf(S);
        if (obz > bz || (obz == bz && obi < bi)) bi = obi;
        const float zlab = found ? zl : ozl;
        const bool counted = (unsigned)label < (unsigned)p.C;          // then one of the two lanes met the label's class
        const int flags = counted ? 1 | (bi == label ? 2 : 0) : 0;
        p.rowst[row] = v4f{M, logS, counted ? (M - zlab) + logS : 0.f, __int_as_float(flags)};
    }
}

__device__ __forceinline__ int logreg_image_offset(int feature, int half) { return 32 * feature + 16 * (half ^ ((feature >> 3) & 1)); }

template <int NT>
__global__ __launch_bounds__(256) void logreg_grad_kernel(LogregArgs p) {
    __shared__ __attribute__((aligned(16))) char image[32 * LOGREG_MAX_DIM];
    __shared__ float zbuf[4][16][64];
    __shared__ v4f st[LOGREG_TILE];
    __shared__ int lab[LOGREG_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int tile = blockIdx.x, part = blockIdx.y, J = p.dim >> 5, groups = p.dim >> 4;
    const long long r_begin = (long long)part * p.per, r_end = min(p.N, r_begin + p.per);
    const int c = tile * LOGREG_TILE + l31;
    const bool c_ok = c < p.C;
    const float bias = c_ok ? p.b[c] : 0.f;
    const v4i *w = p.wp + ((size_t)tile * J * LOGREG_PIECES * 64 + lane) * 2;

    v16f acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = logreg_zero16();
    float gb = 0.f;
    for (long long r0 = r_begin; r0 < r_end; r0 += LOGREG_TILE) {
        __syncthreads();                                                 // the last step's reads are done
        for (int item = tid; item < 8 * groups; item += 256) {           // (a) 16 features of 4 rows -> 16 dwords of the image
            const int cg = item % groups, rg = item / groups;
            v4i x[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long long r = r0 + 4 * rg + q;
                x[q] = v4i{0, 0, 0, 0};
                if (r < r_end) x[q] = *reinterpret_cast<const v4i *>(p.x + (size_t)r * p.dim + 16 * cg);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned o[4];
                probe_transpose4((unsigned)x[0][j], (unsigned)x[1][j], (unsigned)x[2][j], (unsigned)x[3][j], o);
#pragma unroll
                for (int cc = 0; cc < 4; ++cc)                           // row group rg: half rg & 1, dword rg >> 1 of the half
                    *reinterpret_cast<unsigned *>(image + logreg_image_offset(16 * cg + 4 * j + cc, rg & 1) + 4 * (rg >> 1)) = o[cc];
            }
        }
        if (tid < LOGREG_TILE) {
            const long long r = r0 + tid;
            st[tid] = r < r_end ? p.rowst[r] : v4f{0.f, 0.f, 0.f, 0.f};  // flags 0: the row counts for nothing
            lab[tid] = r < r_end ? p.labels[r] : -1;
        }
        {                                                                // (b) this wavefront's share of the logits
            v16f zp = logreg_zero16();
            const bool r_ok = r0 + l31 < r_end;
            const int8_t *src = p.x + (size_t)(r_ok ? r0 + l31 : r_begin) * p.dim + 16 * half;
            for (int j = wave; j < J; j += 4) {
                v4i xa = *reinterpret_cast<const v4i *>(src + 32 * j);
                if (!r_ok) xa = v4i{0, 0, 0, 0};
                v4i b[LOGREG_PIECES][2];
#pragma unroll
                for (int piece = 0; piece < LOGREG_PIECES; ++piece) {
                    b[piece][0] = w[(size_t)(j * LOGREG_PIECES + piece) * 128];
                    b[piece][1] = w[(size_t)(j * LOGREG_PIECES + piece) * 128 + 1];
                }
                const v8bf x0 = logreg_bf16x8(xa[0], xa[1]), x1 = logreg_bf16x8(xa[2], xa[3]);
#pragma unroll
                for (int piece = LOGREG_PIECES - 1; piece >= 0; --piece) {   // the row pass's order exactly
                    zp = logreg_mfma(x0, b[piece][0], zp);
                    zp = logreg_mfma(x1, b[piece][1], zp);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) zbuf[wave][r][lane] = zp[r];
        }
        __syncthreads();
        unsigned gp[16][3];                                              // (c) g, split
        float gsum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ri = (r & 3) + 8 * (r >> 2) + 4 * half;
            const float zs = ((zbuf[0][r][lane] + zbuf[1][r][lane]) + zbuf[2][r][lane]) + zbuf[3][r][lane];
            const v4f sr = st[ri];
            float g = 0.f;
            if (c_ok && (__float_as_int(sr[3]) & 1)) g = expf(((p.xs * zs + bias) - sr[0]) - sr[1]) - (lab[ri] == c ? 1.f : 0.f);
            gsum += g;
            logreg_split3(g, gp[r]);
        }
        gb += gsum;
        v4i ga[LOGREG_PIECES][2];
#pragma unroll
        for (int piece = 0; piece < LOGREG_PIECES; ++piece)
#pragma unroll
            for (int sgm = 0; sgm < 2; ++sgm)
#pragma unroll
                for (int k = 0; k < 4; ++k) ga[piece][sgm][k] = (int)(gp[8 * sgm + 2 * k][piece] | (gp[8 * sgm + 2 * k + 1][piece] << 16));
#pragma unroll
        for (int i = 0; i < NT; ++i) {                                   // (d) this wavefront's feature tiles
            const int t = wave + 4 * i;
            if (t < J) {
                const v4i xb = *reinterpret_cast<const v4i *>(image + logreg_image_offset(32 * t + l31, half));
                const v8bf x0 = logreg_bf16x8(xb[0], xb[1]), x1 = logreg_bf16x8(xb[2], xb[3]);
                v16f tmp = logreg_zero16();
                tmp = logreg_mfma(ga[2][0], x0, tmp);
                tmp = logreg_mfma(ga[2][1], x1, tmp);
                tmp = logreg_mfma(ga[1][0], x0, tmp);
                tmp = logreg_mfma(ga[1][1], x1, tmp);
                tmp = logreg_mfma(ga[0][0], x0, tmp);
                tmp = logreg_mfma(ga[0][1], x1, tmp);
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][r] += tmp[r];
            }
        }
    }
    float *dst = p.pW + ((size_t)part * p.tiles + tile) * LOGREG_TILE * p.dim;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int t = wave + 4 * i;
        if (t < J) {
#pragma unroll
            for (int r = 0; r < 16; ++r) dst[(size_t)((r & 3) + 8 * (r >> 2) + 4 * half) * p.dim + 32 * t + l31] = acc[i][r];
        }
    }
    const float other = __shfl_xor(gb, 32, 64);
    if (wave == 0 && half == 0) p.pb[((size_t)part * p.tiles + tile) * LOGREG_TILE + l31] = gb + other;
}

// blocks [0, nw): grad_W, [nw, nw + nb): grad_b, block nw + nb: loss and correct
__global__ __launch_bounds__(256) void logreg_reduce_kernel(LogregArgs p, unsigned nw, unsigned nb) {
    __shared__ double sl[256];
    __shared__ long long sc[256], sh[256];
    const int tid = threadIdx.x;
    const size_t cpad = (size_t)p.tiles * LOGREG_TILE;
    if (blockIdx.x < nw) {
        const size_t i = (size_t)blockIdx.x * 256 + tid;
        if (i >= (size_t)p.C * p.dim) return;
        float v = 0.f;
        for (int s = 0; s < p.parts; ++s) v += p.pW[(size_t)s * cpad * p.dim + i];
        p.gW[i] = v;
    } else if (blockIdx.x < nw + nb) {
        const size_t i = (size_t)(blockIdx.x - nw) * 256 + tid;
        if (i >= (size_t)p.C) return;
        float v = 0.f;
        for (int s = 0; s < p.parts; ++s) v += p.pb[(size_t)s * cpad + i];
        p.gb[i] = v;
    } else {
        double l = 0.0;
        long long cnt = 0, hit = 0;
        for (long long r = tid; r < p.N; r += 256) {
            const v4f sr = p.rowst[r];
            const int flags = __float_as_int(sr[3]);
            l += (double)sr[2];
            cnt += flags & 1;
            hit += (flags >> 1) & 1;
        }
        sl[tid] = l; sc[tid] = cnt; sh[tid] = hit;
        __syncthreads();
        for (int d = 128; d > 0; d >>= 1) {
            if (tid < d) { sl[tid] += sl[tid + d]; sc[tid] += sc[tid + d]; sh[tid] += sh[tid + d]; }
            __syncthreads();
        }
        if (tid == 0) { p.loss[0] = sl[0]; p.correct[0] = sc[0]; p.correct[1] = sh[0]; }
    }
}
