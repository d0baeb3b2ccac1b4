// ivit_cluster.h — exact integer k-means (include/ivit_cluster.h): the four kernels of a Lloyd iteration over int8 rows and int8
// centroids.  One launch per entry, no workgroup waits for another, no workspace.
//
//   s[r, j] = 2 dot[r, j] - cnorm[j]     assign[r] = the lowest j of the largest s[r, :]     dist2[r] = sum x[r, :]^2 - s[r, assign[r]]
//
// kmeans_assign_kernel<KS, PF>  the hot path, dim = 64 KS: the work shape of search_scan_kernel (ivit_search.h) with the roles renamed.
//   Grid: tiles of 128 rows; a workgroup is four wavefronts that share nothing but the centroid tiles passing through the CU's vector
//   cache (the table is at most K dim bytes and stays in L2): wavefront w owns rows 128 bx + 32 w .. + 31 and keeps them as the B
//   operands of v_mfma_i32_32x32x32_i8 in 8 KS registers for the whole kernel.  It walks the centroids 32 at a time; lane l loads bytes
//   [32 f + 16 (l / 32), + 16) of centroid j0 + l % 32 for every k-step f and, beside them, the norms of the 16 centroids whose scores
//   it will hold.  After 2 KS MFMAs lane l holds, for row l % 32, the dot products with centroids
//   j0 + (r & 3) + 8 (r >> 2) + 4 (l / 32), r = 0 .. 15 — ascending in r.
//   Loads ahead of the MFMAs, three regimes by what fits beside the rows' 8 KS registers (read in the -save-temps assembly):
//     KS <= 7  (PF)   the loads of the NEXT tile (2 KS + 16) are issued, then this tile's MFMAs run back to back with no wait among
//                     them; the wait stands at the rotation an -> a after the tile's keys.  About 24 KS + 50 registers: two
//                     wavefronts per SIMD still fit at KS = 7 (226 + 16), not at KS = 8 (243 + 16), hence the boundary.
//     KS 8 .. 12      all loads of THIS tile are issued together and the MFMAs follow them in order, MFMA f behind
//                     s_waitcnt vmcnt(2 KS - 1 - f): one latency per tile, hidden by the SIMD's other wavefront, not by this one.
//     KS 13 .. 16     the same in two halves of KS loads each (rows + whole tile would be 16 KS > 200 registers).
//   Left to itself the compiler sinks every load of this loop to its use — one 4-register buffer, load, vmcnt(0), MFMA, 2 KS times
//   per tile (the loop is one basic block, unlike search_scan_kernel's, whose filter branch keeps the loads above it) — so each
//   load phase ends in __builtin_amdgcn_sched_barrier(0), a second one follows the MFMAs so that nothing which waits for a load
//   (the rotation, 2^26 - norm) is hoisted among them, and load_tile holds loads only.
//   One running best per lane, one ordered key: t = s + 2^26 lies in (0, 2^27) (|s| < 2^26), so (t << 4) | (15 - r) is a 32-bit key
//   whose maximum over r is the tile's largest score at its lowest centroid; the tile's winner then meets the lane's running
//   64-bit key (t in the high word, 0xFFFFFFFF - j below it) in one comparison.  No LDS, no filter, no compaction.
//   At the end the two lanes of a row exchange their keys (one cross-lane move), the row's sum of squares is taken from the registers
//   it already holds, and lanes 0 .. 31 store assign and dist2.
//   Centroids beyond K in the last tile: the loads are clamped to centroid K - 1, the key keeps the unclamped index, so the copy
//   loses the tie against centroid K - 1 itself and never wins.  Rows beyond the end: clamped on load, never stored.
//
// kmeans_accumulate_kernel<LDS>  sum, count and inertia, modelled on probe_class_kernel (ivit_probe.h).  LDS = true, where K (dim + 1)
//   int32 fit 64 KB: one thread per (row, 16 features) adds into the workgroup's zeroed LDS copy, whose non-zero words are added
//   into the int64 arrays once per PROBE_FLUSH_ROWS rows.  LDS = false: one wavefront per (row, 64 features), lane l feature
//   64 piece + l: the 64-bit global atomic adds of a wavefront are two contiguous runs of 256 B.  The inertia: every thread sums the
//   dist2 of its rows of the part, one wave-reduced 64-bit atomic per wavefront.
// kmeans_update_kernel  one wavefront per centroid, lane p its features 16 p .. + 15: the int64 floor division of the definition,
//   the new bytes stored where count > 0, the exact norm of what the row now holds and "a byte changed" reduced over the wavefront.
// kmeans_norms_kernel  the integer half of gallery_inv_norms_kernel: 16 lanes per centroid.
// Integers throughout: the result depends neither on the grid nor on any order.  Plain vector stores and atomics only, no scratch.
#pragma once
#include "../../include/ivit_cluster.h"
#include "ivit_probe.h"

#define KMEANS_MIN_DIM 64
#define KMEANS_MAX_DIM 1024
#define KMEANS_MAX_K 16384
#define KMEANS_RW 32                               // rows of a wavefront: the N of the MFMA
#define KMEANS_RB (4 * KMEANS_RW)                  // rows of a workgroup
#define KMEANS_TILE 32                             // centroids of a tile: the M of the MFMA
#define KMEANS_PF_MAX_KS 7                         // prefetch the next tile up to dim 448: two wavefronts per SIMD still fit
#define KMEANS_WHOLE_MAX_KS 12                     // up to dim 768 a tile's loads are issued together, above it in two halves
#define KMEANS_BIAS (1 << 26)                      // s + KMEANS_BIAS > 0

struct KMeansAssignArgs {
    const int8_t *x;            // [rows, dim]
    const int8_t *cent;         // [K, dim]
    const int *cnorm;           // [K]
    int *assign;                // [rows]
    int *dist2;                 // [rows] or null
    long long rows;
    int K;
};

template <int KS, bool PF>
__global__ __launch_bounds__(256) void kmeans_assign_kernel(KMeansAssignArgs p) {
    constexpr int NF = 2 * KS, DIM = 64 * KS, PHASES = KS > KMEANS_WHOLE_MAX_KS ? 2 : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const long long q0 = ((long long)blockIdx.x * 4 + wave) * KMEANS_RW;
    if (q0 >= p.rows) return;                                            // whole wavefronts leave: nothing below synchronises a block
    const int last = p.K - 1;

    v4i xf[NF];
    {
        const int8_t *src = p.x + (size_t)min(q0 + l31, p.rows - 1) * DIM + 16 * half;
#pragma unroll
        for (int f = 0; f < NF; ++f) xf[f] = *reinterpret_cast<const v4i *>(src + 32 * f);
    }
    // Loads only, nothing that waits for one: the k-steps [f0, f1) of tile j0 and, with f0 == 0, the norms of the centroids this lane scores
    auto load_tile = [&](int j0, int f0, int f1, v4i (&a)[NF], int (&cn)[16]) {
        if (f0 == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) cn[r] = p.cnorm[min(j0 + ((r & 3) + 8 * (r >> 2) + 4 * half), last)];
        }
        const int8_t *src = p.cent + (size_t)min(j0 + l31, last) * DIM + 16 * half;
#pragma unroll
        for (int f = f0; f < f1; ++f) a[f] = *reinterpret_cast<const v4i *>(src + 32 * f);
    };

    unsigned long long best = 0ull;                                      // no centroid's key: t > 0
    v4i a[NF];
    int bias[16];                                                        // the norms as loaded, then 2^26 - norm: t = 2 dot + bias
    if constexpr (PF) {
        load_tile(0, 0, NF, a, bias);
#pragma unroll
        for (int r = 0; r < 16; ++r) bias[r] = KMEANS_BIAS - bias[r];
    }
    for (int j0 = 0; j0 < p.K; j0 += KMEANS_TILE) {
        v4i an[PF ? NF : 1];
        int bn[PF ? 16 : 1];
        v16i acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0;
        if constexpr (PF) {
            load_tile(j0 + KMEANS_TILE, 0, NF, an, bn);                  // clamped to the last centroid: always inside the arrays
            __builtin_amdgcn_sched_barrier(0);                           // the loads stay issued here (head comment)
#pragma unroll
            for (int f = 0; f < NF; ++f) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[f], xf[f], acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);                           // and the rotation, which waits for them, below
        } else {
#pragma unroll
            for (int ph = 0; ph < PHASES; ++ph) {
                constexpr int FP = NF / PHASES;
                load_tile(j0, ph * FP, (ph + 1) * FP, a, bias);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int f = ph * FP; f < (ph + 1) * FP; ++f) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[f], xf[f], acc, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);                       // the next phase's loads and 2^26 - norm stay below
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) bias[r] = KMEANS_BIAS - bias[r];
        }

        unsigned tk = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned key = ((unsigned)(2 * acc[r] + bias[r]) << 4) | (unsigned)(15 - r);
            tk = key > tk ? key : tk;
        }
        const int r = 15 - (int)(tk & 15u);
        const unsigned j = (unsigned)(j0 + ((r & 3) + 8 * (r >> 2) + 4 * half));
        const unsigned long long key = ((unsigned long long)(tk >> 4) << 32) | (unsigned long long)(0xFFFFFFFFu - j);
        best = key > best ? key : best;
        if constexpr (PF) {
#pragma unroll
            for (int f = 0; f < NF; ++f) a[f] = an[f];
#pragma unroll
            for (int r2 = 0; r2 < 16; ++r2) bias[r2] = KMEANS_BIAS - bn[r2];
        }
    }

    int xx = 0;                                                          // this lane's half of the row's sum of squares
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int b = 0; b < 4; ++b) { const int q = (int)(signed char)((unsigned)xf[f][c] >> (8 * b)); xx += q * q; }
    const unsigned long long other = __shfl_xor(best, 32, 64);
    best = other > best ? other : best;
    xx += __shfl_xor(xx, 32, 64);
    if (lane < KMEANS_RW && q0 + lane < p.rows) {
        p.assign[q0 + lane] = (int)(0xFFFFFFFFu - (unsigned)best);
        if (p.dist2) p.dist2[q0 + lane] = xx - ((int)(unsigned)(best >> 32) - KMEANS_BIAS);
    }
}

struct KMeansAccArgs {
    const int8_t *x;                // [rows, dim]
    const int *assign;              // [rows]
    const int *dist2;               // [rows] or null
    unsigned long long *sum;        // [K, dim]
    unsigned long long *count;      // [K]
    unsigned long long *inertia;    // [1]
    long long rows, per;            // part s covers rows [s * per, min(rows, (s + 1) * per))
    int dim, K;
};

template <bool LDS>
__global__ __launch_bounds__(256) void kmeans_accumulate_kernel(KMeansAccArgs p) {
    extern __shared__ __attribute__((aligned(16))) char kmeans_sm[];
    int *priv = reinterpret_cast<int *>(kmeans_sm);                      // LDS: [K, dim] sums, then [K] counts
    const int nsum = p.K * p.dim, nall = nsum + p.K;
    const long long r_begin = (long long)blockIdx.x * p.per, r_end = min(p.rows, r_begin + p.per);
    if (r_begin >= r_end) return;
    if constexpr (LDS) {
        const int pieces = p.dim >> 4;
        for (long long f0 = r_begin; f0 < r_end; f0 += PROBE_FLUSH_ROWS) {
            const long long f1 = min(r_end, f0 + PROBE_FLUSH_ROWS);
            __syncthreads();
            for (int i = threadIdx.x; i < nall; i += 256) priv[i] = 0;
            __syncthreads();
            const int n = (int)(f1 - f0) * pieces;                        // at most 65 536 * 64
            for (int w = threadIdx.x; w < n; w += 256) {
                const int piece = w % pieces;
                const long long r = f0 + w / pieces;
                const int a = p.assign[r];
                if ((unsigned)a >= (unsigned)p.K) continue;
                const v4i v = *reinterpret_cast<const v4i *>(p.x + (size_t)r * p.dim + 16 * piece);
                const int base = a * p.dim + 16 * piece;
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int b = 0; b < 4; ++b) atomicAdd(priv + base + 4 * j + b, (int)(signed char)((unsigned)v[j] >> (8 * b)));
                if (piece == 0) atomicAdd(priv + nsum + a, 1);
            }
            __syncthreads();
            for (int i = threadIdx.x; i < nall; i += 256) {
                const int s = priv[i];
                if (s) atomicAdd(i < nsum ? p.sum + i : p.count + (i - nsum), (unsigned long long)(long long)s);
            }
        }
    } else {
        const int lane = threadIdx.x & 63, pieces = p.dim >> 6;
        const long long n = (r_end - r_begin) * pieces;                  // (row, 64 features) units of the part
        for (long long u = threadIdx.x >> 6; u < n; u += 4) {
            const long long r = r_begin + u / pieces;
            const int piece = (int)(u % pieces);
            const int a = p.assign[r];                                   // the same for the whole wavefront
            if ((unsigned)a >= (unsigned)p.K) continue;
            const int q = p.x[(size_t)r * p.dim + 64 * piece + lane];
            if (q) atomicAdd(p.sum + (size_t)a * p.dim + 64 * piece + lane, (unsigned long long)(long long)q);
            if (piece == 0 && lane == 0) atomicAdd(p.count + a, 1ull);
        }
    }
    if (p.dist2) {
        long long part = 0;
        for (long long r = r_begin + threadIdx.x; r < r_end; r += 256)
            if ((unsigned)p.assign[r] < (unsigned)p.K) part += p.dist2[r];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d, 64);
        if ((threadIdx.x & 63) == 0 && part) atomicAdd(p.inertia, (unsigned long long)part);
    }
}

__global__ __launch_bounds__(256) void kmeans_update_kernel(const long long *__restrict__ sum, const long long *__restrict__ count, int K, int dim,
                                                            int8_t *cent, int *__restrict__ cnorm, unsigned long long *moved) {
    const int lane = threadIdx.x & 63, j = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= K) return;                                                  // whole wavefronts leave
    int ss = 0, changed = 0;
    if (lane < (dim >> 4)) {
        const size_t o = (size_t)j * dim + 16 * lane;
        const v4i old = *reinterpret_cast<const v4i *>(cent + o);
        v4i now = old;
        const long long n = count[j];
        if (n > 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                unsigned word = 0u;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const long long num = 2 * sum[o + 4 * c + b] + n, den = 2 * n;
                    long long q = num / den;
                    if (num % den < 0) --q;                                  // floor: den > 0
                    word |= ((unsigned)q & 0xFFu) << (8 * b);
                }
                now[c] = (int)word;
            }
            *reinterpret_cast<v4i *>(cent + o) = now;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            changed |= now[c] != old[c];
#pragma unroll
            for (int b = 0; b < 4; ++b) { const int q = (int)(signed char)((unsigned)now[c] >> (8 * b)); ss += q * q; }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        ss += __shfl_xor(ss, d, 64);
        changed |= __shfl_xor(changed, d, 64);
    }
    if (lane == 0) {
        cnorm[j] = ss;
        if (changed) atomicAdd(moved, 1ull);
    }
}

__global__ __launch_bounds__(256) void kmeans_norms_kernel(const int8_t *__restrict__ cent, int K, int dim, int *__restrict__ cnorm) {
    const int sub = threadIdx.x & 15, nchunks = dim >> 4;
    const int j = (int)blockIdx.x * 16 + (threadIdx.x >> 4);             // the 16 lanes of a centroid stay or leave together
    if (j >= K) return;
    const v4i *row = reinterpret_cast<const v4i *>(cent + (size_t)j * dim);
    int ss = 0;
    for (int c = sub; c < nchunks; c += 16) {
        const v4i v = row[c];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int b = 0; b < 4; ++b) { const int q = (int)(signed char)((unsigned)v[i] >> (8 * b)); ss += q * q; }
    }
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) ss += __shfl_xor(ss, d, 16);
    if (sub == 0) cnorm[j] = ss;
}
