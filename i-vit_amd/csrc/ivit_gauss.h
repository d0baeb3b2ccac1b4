// ivit_gauss.h — novelty scores (include/ivit_gauss.h): the squared Mahalanobis distance of int8 feature rows to the nearest class mean
// of a shared-covariance Gaussian model, and that class.  The model is a TABLE of R + C float rows over the features' integers x:
//
//   z[r, k] = Wh[k, :] . x[r, :] + t[k]     q[r] = sum_k z[r, k]^2          the R whitening rows: the squared distance to the pooled mean
//   s[r, c] = Wc[c, :] . x[r, :] + bc[c]    best[r] = max_c s[r, c], cls[r] its smallest index          dist[r] = q[r] - best[r]
//
// Neither the [N, R] whitened rows nor the [N, C] scores are ever written: a whitening tile leaves ONE float per row, the class tiles
// one (value, index) per row and part.
//
// Operands.  ivit_logreg.h's argument: an int8 feature is exact in bf16, a float is the exact sum of three bf16 pieces (logreg_split3),
//   the product of a piece and an int8 value has at most 16 significant bits, so every product inside v_mfma_f32_32x32x16_bf16 is
//   exact and only the fp32 accumulation rounds.  The model is constant across calls (unlike the logistic probe's W), so the pieces
//   are made once, by ivit_gauss_prepare, and a score call reads them as they lie.
// gauss_prepare_kernel  the table as tiles of 32 rows: the R / 32 whitening tiles first, then ceil(C / 32) class tiles whose rows >= C
//   are zeros.  Block (tile, pair-step j of 32 features, piece) holds, for lane l, the 16 bf16 of table row 32 tile + l % 32, features
//   32 j + 16 (l / 32) .. + 15 — logreg_pieces_kernel's block, 32 bytes per lane; a STEP of the scorer is two pair-steps (64 features),
//   GAUSS_STEP_V4 16-byte words.  Behind the pieces: the vector, R + 32 ceil(C / 32) floats — t, then bc with -inf on the padding.
// gauss_score_kernel<KS>  dim = 64 KS.  Grid (row blocks of 128, parts of the table); a workgroup is four wavefronts of 32 rows, a
//   wavefront keeps its rows as int8 in 8 KS registers for the whole kernel (the MFMA's B operand, converted per pair-step:
//   kmeans_assign_kernel's work shape) and walks the tiles [part * per, (part + 1) * per) of the table.  No LDS, no scratch: the four
//   wavefronts of a workgroup read the same pieces and meet in the vector L1.
//   Prefetch: the table is one run of steps (tile-major), so the pieces of step m + 1 (twelve 16-byte loads per lane) are requested
//   before the twelve MFMAs of step m are issued.  At KS = 1 a step IS a tile — the whole next tile is in flight under this tile's
//   MFMAs; at KS >= 2 the last step of a tile prefetches the first of the next.  The step behind a part's last is the next part's first
//   (read, not used); behind the table's last the address is clamped to the last.
//   Order: pair-step j adds into accumulator set j & 1, the small pieces first; the sets meet as s0 + s1, then the vector's entry is
//   added.  The same for every tile, so a value's bits do not depend on the part its tile falls in.  After a tile lane l holds, for
//   row l % 32, the table rows 32 tile + (r & 3) + 8 (r >> 2) + 4 (l / 32), r = 0 .. 15, ascending in r.
//   A whitening tile: the lane squares and sums its 16 components in that order, the two lanes of a row add (a + b is commutative:
//   both compute the same bits), lane l < 32 stores the row's float at qpart[tile][row].
//   A class tile: one running (value, index) per lane under a strict compare — ascending classes, so the first of equal scores stays.
//   When the part is done the two lanes of a row meet (the larger value, the smaller index on a tie) and lane l < 32 stores
//   pbest[part][row], pcls[part][row]; a part without a class tile stores (-inf, INT_MAX).
// gauss_finish_kernel  one thread per row: q = the tiles' partials added in ascending tile order; (best, cls) from (-inf, 0) over the
//   parts in ascending order under a strict compare; dist = q - best.  Hence q, best, cls and dist hold the same bits for every
//   `splits`, every grid and every call; all classes at -inf give cls 0, best -inf, dist +inf and no NaN.
// No atomics.  Plain vector stores only.
#pragma once
#include "../../include/ivit_gauss.h"
#include "ivit_logreg.h"

#define GAUSS_MIN_DIM 64
#define GAUSS_MAX_DIM 1024
#define GAUSS_MAX_CLASSES 65536
#define GAUSS_MAX_SPLITS 256
#define GAUSS_TILE 32                               // table rows of a tile, feature rows of a wavefront: the M and N of the MFMA
#define GAUSS_RB 128                                // rows of a workgroup
#define GAUSS_STEP_V4 (2 * LOGREG_PIECES * 64 * 2)  // 16-byte words of a step: two pair-steps x three pieces x 64 lanes x 32 bytes

struct GaussArgs {
    const float *Wh, *t, *Wc, *bc;  // prepare: the caller's model
    v4i *pieces;                    // the prepared model: [tiles][dim / 64] steps
    float *vec;                     //   behind them: t [R], bc [32 ceil(C / 32)]
    const int8_t *x;                // [N, dim]
    float *qpart, *pbest;           // workspace: [R / 32][N], [parts][N]
    int *pcls;                      //            [parts][N]
    float *q, *best, *dist;
    int *cls;
    long long N;
    int dim, R, C, qtiles, tiles, per, parts;   // part s covers the tiles [s per, min(tiles, (s + 1) per))
};

// one thread per (tile, pair-step, lane); the first R + 32 ceil(C / 32) threads write the vector too
__global__ __launch_bounds__(256) void gauss_prepare_kernel(GaussArgs p) {
    const int J = p.dim >> 5;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)p.tiles * J * 64) return;
    if (t < (long long)p.tiles * GAUSS_TILE) {
        const int c = (int)t - p.R;
        p.vec[t] = c < 0 ? p.t[t] : c < p.C ? p.bc[c] : -__builtin_inff();
    }
    const int lane = (int)(t & 63), j = (int)((t >> 6) % J), tile = (int)((t >> 6) / J);
    const int row = tile * GAUSS_TILE + (lane & 31);
    const float *src = row < p.R ? p.Wh + (size_t)row * p.dim : row - p.R < p.C ? p.Wc + (size_t)(row - p.R) * p.dim : nullptr;
    unsigned pc[16][3];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        v4f w = v4f{0.f, 0.f, 0.f, 0.f};
        if (src) w = *reinterpret_cast<const v4f *>(src + 32 * j + 16 * (lane >> 5) + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) logreg_split3(w[e], pc[4 * q + e]);
    }
    v4i *dst = p.pieces + ((size_t)(tile * J + j) * LOGREG_PIECES * 64 + lane) * 2;
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

struct GaussStep { v4i a[2][LOGREG_PIECES][2]; };   // a lane's operands of one step: [pair-step][piece][k-step]

__device__ __forceinline__ GaussStep gauss_load_step(const v4i *w) {
    GaussStep s;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int piece = 0; piece < LOGREG_PIECES; ++piece) {
            s.a[j][piece][0] = w[(size_t)(j * LOGREG_PIECES + piece) * 128];
            s.a[j][piece][1] = w[(size_t)(j * LOGREG_PIECES + piece) * 128 + 1];
        }
    return s;
}

template <int KS>
__global__ __launch_bounds__(256) void gauss_score_kernel(GaussArgs p) {
    constexpr int DIM = 64 * KS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const long long r0 = ((long long)blockIdx.x * 4 + wave) * GAUSS_TILE;
    if (r0 >= p.N) return;                                               // whole wavefronts leave: nothing below synchronises a block
    const long long row = min(r0 + l31, p.N - 1);                        // rows beyond the end: clamped on load, never stored
    const bool writer = half == 0 && r0 + l31 < p.N;
    v4i xr[2 * KS];
    {
        const int8_t *src = p.x + (size_t)row * DIM + 16 * half;
#pragma unroll
        for (int j = 0; j < 2 * KS; ++j) xr[j] = *reinterpret_cast<const v4i *>(src + 32 * j);
    }
    const int part = blockIdx.y, t_begin = part * p.per, t_end = min(p.tiles, t_begin + p.per);
    const v4i *w = p.pieces + (size_t)t_begin * KS * GAUSS_STEP_V4 + lane * 2;
    const v4i *const w_last = p.pieces + ((size_t)p.tiles * KS - 1) * GAUSS_STEP_V4 + lane * 2;
    const float NEG = -__builtin_inff();
    float bv = NEG;
    int bi = 0x7fffffff;
    GaussStep cur = gauss_load_step(w);
    for (int tile = t_begin; tile < t_end; ++tile) {
        v4f add[4];                                                      // the vector's entries of this lane's 16 table rows
#pragma unroll
        for (int g = 0; g < 4; ++g) add[g] = *reinterpret_cast<const v4f *>(p.vec + tile * GAUSS_TILE + 8 * g + 4 * half);
        v16f acc[2] = {logreg_zero16(), logreg_zero16()};
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            w += GAUSS_STEP_V4;
            const GaussStep nxt = gauss_load_step(w < w_last ? w : w_last);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const v4i xv = xr[2 * k + j];
                const v8bf x0 = logreg_bf16x8(xv[0], xv[1]), x1 = logreg_bf16x8(xv[2], xv[3]);
#pragma unroll
                for (int piece = LOGREG_PIECES - 1; piece >= 0; --piece) {   // the small pieces first
                    acc[j] = logreg_mfma(cur.a[j][piece][0], x0, acc[j]);
                    acc[j] = logreg_mfma(cur.a[j][piece][1], x1, acc[j]);
                }
            }
            cur = nxt;
        }
        if (tile < p.qtiles) {                                           // wave-uniform
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float z = (acc[0][r] + acc[1][r]) + add[r >> 2][r & 3];
                s += z * z;
            }
            const float o = __shfl_xor(s, 32, 64);
            if (writer) p.qpart[(size_t)tile * p.N + row] = s + o;
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float s = (acc[0][r] + acc[1][r]) + add[r >> 2][r & 3];
                const int c = (tile - p.qtiles) * GAUSS_TILE + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (s > bv) { bv = s; bi = c; }                          // ascending classes: the first of equal scores stays
            }
        }
    }
    const float ov = __shfl_xor(bv, 32, 64);
    const int oi = __shfl_xor(bi, 32, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    if (writer) {
        p.pbest[(size_t)part * p.N + row] = bv;
        p.pcls[(size_t)part * p.N + row] = bi;
    }
}

__global__ __launch_bounds__(256) void gauss_finish_kernel(GaussArgs p) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= p.N) return;
    float q = p.qpart[r];
    for (int tile = 1; tile < p.qtiles; ++tile) q += p.qpart[(size_t)tile * p.N + r];
    float best = -__builtin_inff();
    int cls = 0;
    for (int s = 0; s < p.parts; ++s) {
        const float v = p.pbest[(size_t)s * p.N + r];
        if (v > best) { best = v; cls = p.pcls[(size_t)s * p.N + r]; }
    }
    p.q[r] = q;
    p.best[r] = best;
    p.cls[r] = cls;
    p.dist[r] = q - best;
}
