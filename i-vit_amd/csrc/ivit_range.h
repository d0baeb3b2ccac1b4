// ivit_range.h — range search (include/ivit_range.h): every gallery row whose score against a query reaches a threshold, in CSR form,
// the gallery read twice, the scores never written.  Deterministic without a sort and without an atomic: the first pass counts the
// hits of every (query, part of the gallery), an exclusive scan in query-major order turns the counts into positions, the second pass
// — THE SAME kernel source, so that the two cannot disagree about a hit — writes every hit at its position.  Takes nothing from
// ivit_search.h but the work shape (SEARCH_QW, SEARCH_QB, SEARCH_TILE, SEARCH_PF_MAX_KS) and topk_value.
//
//   value   v[b, g] = fl32(topk_value(dot[b, g], weight[g]) * qweight[b]): one conversion and two fp32 multiplies in this order, a NULL
//           weight / qweight a multiplication by 1.0f (the same bits, -0.0 included).
//   hit     v >= threshold (the IEEE comparison) and, with triangle, index_base + g > query_base + b.
//
// range_scan_kernel<KS, PF, FILL>  dim = 64 KS.  The geometry of search_scan_kernel: grid (tiles of 128 queries) x (parts of the
//   gallery); four wavefronts per workgroup that share nothing but the gallery rows passing through the CU's vector cache; wavefront
//   w keeps queries 128 bx + 32 w .. + 31 as the B operands of v_mfma_i32_32x32x32_i8 for the whole kernel and walks its part 32 rows
//   at a time, the loads of the NEXT tile issued before the MFMAs of this one (PF; off above dim 512).  After 2 KS MFMAs lane l holds,
//   for query l % 32, the 16 dot products of rows (r & 3) + 8 (r >> 2) + 4 (l / 32), r = 0 .. 15, and builds a 16-bit mask of its
//   hits: the row inside the part, v >= threshold, the triangle.  When no lane has a hit the tile is done.  No LDS, no atomics.
//   Count (FILL = false): a counter per lane; at the end the two lanes of a query add through one cross-lane exchange and lanes
//     0 .. 31 store cnt[query * parts + part], one plain store.
//   Fill (FILL = true): an int64 cursor per lane, from off[query * parts + part].  Per tile with a hit, ONE exchange of the mask with
//     lane l ^ 32 (executed by all 64 lanes: the branch is wave-uniform) gives a lane its partner's hits.  Rows 8 j .. 8 j + 3 (group j
//     of half 0) precede rows 8 j + 4 .. 8 j + 7 (group j of half 1), so a lane's position for bit r of its group j is the cursor, plus
//     both lanes' hits in groups < j, plus the partner's group j if this lane is half 1, plus its own hits of group j below r: ascending
//     g with no sort.  A store happens only at 0 <= p < capacity (one unsigned comparison: whatever the workspace holds, nothing is
//     written outside).  Both lanes advance the cursor by both counts.
//   Triangle: a wavefront starts at its first tile that is not wholly at or below its diagonal (index_base + g0 + 31 <= query_base +
//     q0 for every tile before): a self-join loads about half the tiles.  Tiles the diagonal crosses are masked per element.
//   Rows and queries beyond the end: the loads are clamped to the last row / query (always inside the arrays); a row beyond the
//   part's end and a query beyond nq are never counted or stored.
//
// range_block_sums_kernel / range_scan_sums_kernel / range_offsets_kernel  the exclusive scan of the n = nq * parts counts into int64
//   offsets, three ordinary launches: the sum of every block of RANGE_SCAN_BLOCK counts; ONE workgroup turns the block sums into their
//   exclusive scan and writes the total to row_ptr[nq]; every block scans its own counts again from its base, writes off[i] and, where
//   i is a query's first part, row_ptr[query].  No look-back chain: no workgroup waits for another.
// Plain vector stores only, no scratch.
#pragma once
#include "../../include/ivit_range.h"
#include "ivit_search.h"

#define RANGE_SCAN_PER 16                              // counts of a thread
#define RANGE_SCAN_BLOCK (256 * RANGE_SCAN_PER)        // counts of a block

struct RangeArgs {
    const int8_t *query;        // [nq, dim]
    const int8_t *gallery;      // [rows, dim]
    const float *weight;        // [rows] or null
    const float *qweight;       // [nq] or null
    int *cnt;                   // [nq, parts]: written by the count pass
    const long long *off;       // [nq, parts]: read by the fill pass
    int *idx;                   // [capacity]
    float *val;                 // [capacity] or null
    long long rows, per;        // part s covers rows [s * per, min(rows, (s + 1) * per))
    long long capacity;
    float threshold;
    int nq, index_base, query_base, triangle, parts;
};

template <int KS, bool PF, bool FILL>
__global__ __launch_bounds__(256) void range_scan_kernel(RangeArgs p) {
    constexpr int NF = 2 * KS, DIM = 64 * KS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const long long q0 = ((long long)blockIdx.x * 4 + wave) * SEARCH_QW;
    if (q0 >= p.nq) return;                                              // whole wavefronts leave: nothing below synchronises a block
    const bool live = q0 + l31 < p.nq;                                   // this lane's query exists
    const long long qrow = min(q0 + l31, (long long)p.nq - 1);

    const long long g_begin = (long long)blockIdx.y * p.per, g_end = min(p.rows, g_begin + p.per);
    const long long last_row = p.rows - 1;
    long long g_first = g_begin;
    if (p.triangle) {                                                    // tiles wholly at or below the wavefront's diagonal are skipped
        const long long d = ((long long)p.query_base + q0) - ((long long)p.index_base + g_begin) - (SEARCH_TILE - 1);
        if (d >= 0) g_first = g_begin + (d / SEARCH_TILE + 1) * SEARCH_TILE;
    }

    v4i qf[NF];
    {
        const int8_t *src = p.query + (size_t)qrow * DIM + 16 * half;
#pragma unroll
        for (int f = 0; f < NF; ++f) qf[f] = *reinterpret_cast<const v4i *>(src + 32 * f);
    }
    const float qw = p.qweight ? p.qweight[qrow] : 1.0f;
    const float thr = p.threshold;
    auto load_tile = [&](long long g0, v4i (&a)[NF], float (&w)[16]) {
        const int8_t *src = p.gallery + (size_t)min(g0 + l31, last_row) * DIM + 16 * half;
#pragma unroll
        for (int f = 0; f < NF; ++f) a[f] = *reinterpret_cast<const v4i *>(src + 32 * f);
#pragma unroll
        for (int r = 0; r < 16; ++r) w[r] = p.weight ? p.weight[min(g0 + ((r & 3) + 8 * (r >> 2) + 4 * half), last_row)] : 1.0f;
    };

    // the diagonal as seen from this lane's query, in rows of the gallery; without the triangle so far below that every row is above it.
    // Taken out of the loop so that NO BRANCH stands between a tile's MFMAs and the reads of their accumulators: with `if (triangle)`
    // there, the compiler put the branch behind the last MFMA and only one wait state before v_accvgpr_read of its last register, which
    // then still held the sum of the MFMA before (seen on an MI355X: one value of a tile was the dot product over the first 32 bytes).
    const long long dq = p.triangle ? ((long long)p.query_base + q0 + l31) - (long long)p.index_base : -(1ll << 40);

    int count = 0;                                                       // FILL = false: this lane's hits
    long long cursor = 0;                                                // FILL = true: the position of the query's next hit
    if constexpr (FILL) cursor = p.off[(size_t)qrow * p.parts + blockIdx.y];

    v4i a[NF];
    float w[16];
    if constexpr (PF) load_tile(min(g_first, last_row), a, w);
    for (long long g0 = g_first; g0 < g_end; g0 += SEARCH_TILE) {
        v4i an[PF ? NF : 1];
        float wn[PF ? 16 : 1];
        if constexpr (PF) load_tile(g0 + SEARCH_TILE, an, wn);           // clamped to the last row: always inside the arrays
        else load_tile(g0, a, w);
        v16i acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0;
#pragma unroll
        for (int f = 0; f < NF; ++f) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[f], qf[f], acc, 0, 0, 0);

        const int nrow = live ? (int)min((long long)SEARCH_TILE, g_end - g0) : 0;      // rows of this tile inside the part
        // a row of the tile is above the diagonal when row > (query_base + b) - (index_base + g0); -1 lets every row pass
        const int diag = (int)max(-1ll, min((long long)SEARCH_TILE, dq - g0));
        float v[16];
        unsigned mask = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
            v[r] = __fmul_rn(topk_value(acc[r], w[r]), qw);
            if (row < nrow && row > diag && v[r] >= thr) mask |= 1u << r;
        }
        if (__any(mask != 0u)) {
            if constexpr (FILL) {
                const unsigned other = (unsigned)__shfl_xor((int)mask, 32);          // the partner's hits: every lane is here
                const int c0 = (int)(p.index_base + g0);                             // index_base + rows <= 2^31 - 1
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (mask & (1u << r)) {
                        const int j = r >> 2;
                        const unsigned before = (1u << (4 * j)) - 1u, group = 0xFu << (4 * j);
                        const int ahead = __popc(mask & before) + __popc(other & before) + (half ? __popc(other & group) : 0) +
                                          __popc(mask & group & ((1u << r) - 1u));
                        const long long pos = cursor + ahead;
                        if ((unsigned long long)pos < (unsigned long long)p.capacity) {
                            p.idx[pos] = c0 + (r & 3) + 8 * j + 4 * half;
                            if (p.val) p.val[pos] = v[r];
                        }
                    }
                }
                cursor += __popc(mask) + __popc(other);
            } else {
                count += __popc(mask);
            }
        }
        if constexpr (PF) {
#pragma unroll
            for (int f = 0; f < NF; ++f) a[f] = an[f];
#pragma unroll
            for (int r = 0; r < 16; ++r) w[r] = wn[r];
        }
    }

    if constexpr (!FILL) {
        count += __shfl_xor(count, 32);                                  // the two lanes of a query
        if (half == 0 && live) p.cnt[(size_t)(q0 + l31) * p.parts + blockIdx.y] = count;
    }
}

// the inclusive scan of one value per thread over a block of 256 (four wavefronts), and the block's total
__device__ __forceinline__ long long range_block_scan(long long x, long long *total) {
    __shared__ long long wave_sum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    __syncthreads();                                                     // a second call: the readers of the first are through
    if (lane == 63) wave_sum[wave] = x;
    __syncthreads();
    long long base = 0, all = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long s = wave_sum[i];
        if (i < wave) base += s;
        all += s;
    }
    *total = all;
    return x + base;
}

__global__ __launch_bounds__(256) void range_block_sums_kernel(const int *__restrict__ cnt, long long n, long long *__restrict__ bsum) {
    const long long i0 = (long long)blockIdx.x * RANGE_SCAN_BLOCK + (long long)threadIdx.x * RANGE_SCAN_PER;
    long long s = 0;
#pragma unroll
    for (int i = 0; i < RANGE_SCAN_PER; ++i) s += i0 + i < n ? (long long)cnt[i0 + i] : 0ll;
    long long total;
    range_block_scan(s, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: the block sums in place into their exclusive scan, 256 at a time with a carry; the total to *total_out
__global__ __launch_bounds__(256) void range_scan_sums_kernel(long long *__restrict__ bsum, long long nb, long long *__restrict__ total_out) {
    long long carry = 0;
    for (long long b0 = 0; b0 < nb; b0 += 256) {
        const long long i = b0 + threadIdx.x;
        const long long x = i < nb ? bsum[i] : 0ll;
        long long total;
        const long long incl = range_block_scan(x, &total);
        if (i < nb) bsum[i] = carry + incl - x;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

__global__ __launch_bounds__(256) void range_offsets_kernel(const int *__restrict__ cnt, const long long *__restrict__ bsum, long long n, int parts,
                                                            long long *__restrict__ off, long long *__restrict__ row_ptr) {
    const long long i0 = (long long)blockIdx.x * RANGE_SCAN_BLOCK + (long long)threadIdx.x * RANGE_SCAN_PER;
    int c[RANGE_SCAN_PER];
    long long s = 0;
#pragma unroll
    for (int i = 0; i < RANGE_SCAN_PER; ++i) {
        c[i] = i0 + i < n ? cnt[i0 + i] : 0;
        s += c[i];
    }
    long long total;
    long long at = bsum[blockIdx.x] + range_block_scan(s, &total) - s;   // the exclusive offset of this thread's first count
#pragma unroll
    for (int i = 0; i < RANGE_SCAN_PER; ++i) {
        if (i0 + i < n) {
            off[i0 + i] = at;
            if ((i0 + i) % parts == 0) row_ptr[(i0 + i) / parts] = at;
        }
        at += c[i];
    }
}
