// ivit_search.h — gallery search (include/ivit_search.h): the k best rows of an int8 gallery for every int8 query, the gallery read
// once, the scores never written.  Three kernels, two launches per search, no workgroup waits for another.
//
//   value   v[b, g] = fl32(fl32(dot[b, g]) * weight[g]), dot the exact int32 product of query b and gallery row g: topk_value of
//           ivit_topk.h (a NULL weight is a multiplication by 1.0f: the same bits).
//   order   topk_key of ivit_topk.h, the library's ONE definition: descending by value, -0.0 equal to +0.0, equal values by ascending
//           index.  The keys here are that key PACKED (search_pack): the high word unchanged; the low word 0xFFFFFFFF - c always has
//           bit 31 set (c < 2^31), so it is shifted left by one — the order among distinct c is unchanged — and bit 0 says "the value
//           was -0.0", which the high word (zero canonicalised) cannot.  A packed key therefore holds everything the outputs need: the
//           index (search_key_index) and every bit of the value (search_key_value).  0 is no row's key and stands for "nothing".
//
// search_scan_kernel<KS, PF>  the first phase, dim = 64 KS.  Grid (tiles of 128 queries) x (parts of the gallery); a workgroup is four
//   wavefronts that share nothing but the gallery rows passing through the CU's vector cache: wavefront w owns queries
//   128 bx + 32 w .. + 31 and keeps them as the B operands of v_mfma_i32_32x32x32_i8 in 8 KS registers for the whole kernel.  It
//   walks its part of the gallery 32 rows at a time; lane l loads bytes [32 f + 16 (l / 32), + 16) of row l % 32 for every k-step f
//   (16-byte loads; a tile's rows are one contiguous run), the loads of the NEXT tile issued before the MFMAs of this one (PF; off
//   above dim 512, where twice the tile does not fit beside the queries).  After 2 KS MFMAs lane l holds, for query l % 32, the 16 dot
//   products of rows (r & 3) + 8 (r >> 2) + 4 (l / 32), r = 0 .. 15.
//   Filter: a query's threshold is its current k-th best key (0 until k rows were seen) and, beside it, that key's VALUE tv: a
//   score passes only if v >= tv (one convert, one multiply, one compare per score; -inf until there is a k-th).  When no lane of the
//   wavefront has a survivor the tile is done.  Otherwise the survivors' keys are built, compared with the threshold exactly, and
//   appended to the lane's OWN pending run in LDS (a query has two lanes, each its run of CL slots and its count in a register: no
//   atomics).  When some lane's run could not take another 16 keys the wavefront compacts ALL its queries (search_compact_all: lane q
//   alone sorts the k best of query q's nslot slots — the kcap best, then the two runs; unused slots hold 0 — to the front and zeroes
//   the rest), every lane takes its query's new threshold from slot k - 1 and empties its run.  Every score may survive (a gallery in
//   ascending order of its score): then every lane appends 16 keys per tile and the wavefront compacts every (CL - 15) / 16 tiles,
//   which is slow and correct.  nslot = 64 (kcap 16, CL 24) for k <= 16, 128 (kcap 64, CL 32) above.
//   At the end of its part a wavefront compacts once more and lanes 0 .. k-1 store each query's k keys, best first, to
//   ws[(query * parts + part) * k ..]: a part of fewer than k rows pads with 0.
//   Rows and queries beyond the end: the loads are clamped to the last row / query (always inside the arrays); a row beyond the
//   part's end never passes the filter, a query beyond nq is never stored.
//
// search_select_kernel<PAIRS, PER>  the second phase, one wavefront per query: the k best of n keys by the rounds of logits_topk_kernel
//   (round j: the wave-wide maximum of the keys below round j - 1's winner), then idx / val from the packed keys.  PER = 16 / 64: a
//   lane holds keys l, l + 64, ... in registers, read once (n <= 1024 / 4096); PER = 0: every round rescans the n keys from memory
//   (L2-resident).  PAIRS = false reads ws (n = parts * k); PAIRS = true is ivit_search_merge: the keys are built from
//   (val_in, idx_in) — topk_key(1, val, idx), the multiplication by fl32(1) being exact.
//
// gallery_inv_norms_kernel  16 lanes per row: the exact integer sum of squares, the correctly rounded fp64 root (the residual step
//   of features_f32_kernel<UNIT>), the fp64 reciprocal, one rounding to fp32; a row of zeros gives +0.0f.
// Plain vector stores only, no scratch.
#pragma once
#include "../../include/ivit_search.h"
#include "ivit_topk.h"

#define SEARCH_MAX_K 64
#define SEARCH_MIN_DIM 64
#define SEARCH_MAX_DIM 1024
#define SEARCH_QW 32                               // queries of a wavefront: the N of the MFMA
#define SEARCH_QB (4 * SEARCH_QW)                  // queries of a workgroup
#define SEARCH_TILE 32                             // gallery rows of a tile: the M of the MFMA
#define SEARCH_PF_MAX_KS 8                         // prefetch the next tile up to dim 512

__host__ __device__ __forceinline__ int search_nslot(int k) { return k <= 16 ? 64 : 128; }
__host__ __device__ __forceinline__ int search_kcap(int k) { return k <= 16 ? 16 : 64; }
// bytes between two queries' slots: one spare slot, so that the 32 queries of a wavefront start in different banks
__host__ __device__ __forceinline__ int search_qstride(int k) { return search_nslot(k) * 8 + 8; }
__host__ __device__ __forceinline__ size_t search_lds_bytes(int k) { return (size_t)SEARCH_QB * search_qstride(k); }

__device__ __forceinline__ unsigned long long search_pack(unsigned long long key, unsigned vbits) {
    const unsigned lo = (unsigned)key;                                   // 0xFFFFFFFF - c: bit 31 is set for every c < 2^31
    return (key & 0xFFFFFFFF00000000ull) | (unsigned long long)((lo << 1) | (vbits == 0x80000000u ? 1u : 0u));
}
__device__ __forceinline__ int search_key_index(unsigned long long p) { return (int)(0x7FFFFFFFu - ((unsigned)p >> 1)); }
__device__ __forceinline__ float search_key_value(unsigned long long p) {
    unsigned u = (unsigned)(p >> 32);
    u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;                      // topk_key's map, inverted
    if ((unsigned)p & 1u) u = 0x80000000u;                               // a zero that was -0.0
    return __uint_as_float(u);
}

struct SearchArgs {
    const int8_t *query;        // [nq, dim]
    const int8_t *gallery;      // [rows, dim]
    const float *weight;        // [rows] or null
    unsigned long long *ws;     // [nq, parts, k]
    long long rows, per;        // part s covers rows [s * per, min(rows, (s + 1) * per))
    int nq, k, index_base, parts;
};

// the wavefront's accesses to its own LDS, ordered: writes of some lanes are read by others
__device__ __forceinline__ void search_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Compaction of all 32 queries of a wavefront at once, lane q < 32 working ALONE on query q's nslot slots (unused ones hold 0): k rounds of
// selection by swapping — round j finds the largest of slots j .. nslot - 1 and swaps it into slot j — then every slot behind the k-th
// is zeroed.  Afterwards slots 0 .. k-1 hold the k best, best first (0 beyond what there is).  No lane reads what another wrote inside:
// the two fences order it against the appends before and the readers behind.  The scan's loads are independent (LDS pipelines them); a
// wave-wide maximum per rank and query instead (the rounds of logits_topk_kernel, one query at a time) is six dependent cross-lane
// exchanges per rank: the whole search was 3.1 x slower with it at 131 072 rows (profiles/README.md, "Gallery search").
__device__ __forceinline__ void search_compact_all(char *wbase, int qstride, int nslot, int k, int lane) {
    search_wave_sync();
    if (lane < SEARCH_QW) {
        unsigned long long *s = reinterpret_cast<unsigned long long *>(wbase + (size_t)lane * qstride);
        for (int j = 0; j < k; ++j) {
            unsigned long long best = s[j];
            int pos = j;
#pragma unroll 8
            for (int i = j + 1; i < nslot; ++i) {
                const unsigned long long e = s[i];
                if (e > best) { best = e; pos = i; }
            }
            if (best == 0ull) break;                                     // nothing is left: the rest is zeros already
            const unsigned long long t = s[j];
            s[pos] = t;
            s[j] = best;
        }
        for (int i = k; i < nslot; ++i) s[i] = 0ull;
    }
    search_wave_sync();
}

template <int KS, bool PF>
__global__ __launch_bounds__(256) void search_scan_kernel(SearchArgs p) {
    constexpr int NF = 2 * KS, DIM = 64 * KS;
    extern __shared__ __attribute__((aligned(16))) char search_sm[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const long long q0 = ((long long)blockIdx.x * 4 + wave) * SEARCH_QW;
    if (q0 >= p.nq) return;                                              // whole wavefronts leave: nothing below synchronises a block
    const int k = p.k, nslot = search_nslot(k), kcap = search_kcap(k), CL = (nslot - kcap) >> 1, qstride = search_qstride(k);
    char *wbase = search_sm + (size_t)wave * SEARCH_QW * qstride;
    for (int i = lane; i < SEARCH_QW * (nslot + 1); i += 64) reinterpret_cast<unsigned long long *>(wbase)[i] = 0ull;
    const unsigned long long *best = reinterpret_cast<const unsigned long long *>(wbase + (size_t)l31 * qstride);         // this lane's query
    unsigned long long *pend = reinterpret_cast<unsigned long long *>(wbase + (size_t)l31 * qstride) + kcap + half * CL;   // this lane's run
    search_wave_sync();

    const long long g_begin = (long long)blockIdx.y * p.per, g_end = min(p.rows, g_begin + p.per);
    const long long last_row = p.rows - 1;

    v4i qf[NF];
    {
        const int8_t *src = p.query + (size_t)min(q0 + l31, (long long)p.nq - 1) * DIM + 16 * half;
#pragma unroll
        for (int f = 0; f < NF; ++f) qf[f] = *reinterpret_cast<const v4i *>(src + 32 * f);
    }
    auto load_tile = [&](long long g0, v4i (&a)[NF], float (&w)[16]) {
        const int8_t *src = p.gallery + (size_t)min(g0 + l31, last_row) * DIM + 16 * half;
#pragma unroll
        for (int f = 0; f < NF; ++f) a[f] = *reinterpret_cast<const v4i *>(src + 32 * f);
#pragma unroll
        for (int r = 0; r < 16; ++r) w[r] = p.weight ? p.weight[min(g0 + ((r & 3) + 8 * (r >> 2) + 4 * half), last_row)] : 1.0f;
    };

    unsigned long long thr = 0ull;                                       // this lane's query: its k-th best key so far
    float tv = -__builtin_inff();                                        // and that key's value
    int cnt = 0;                                                         // keys in this lane's run

    v4i a[NF];
    float w[16];
    if constexpr (PF) load_tile(min(g_begin, last_row), a, w);
    for (long long g0 = g_begin; g0 < g_end; g0 += SEARCH_TILE) {
        v4i an[PF ? NF : 1];
        float wn[PF ? 16 : 1];
        if constexpr (PF) load_tile(g0 + SEARCH_TILE, an, wn);           // clamped to the last row: always inside the arrays
        else load_tile(g0, a, w);
        v16i acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0;
#pragma unroll
        for (int f = 0; f < NF; ++f) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[f], qf[f], acc, 0, 0, 0);

        const int nrow = (int)min((long long)SEARCH_TILE, g_end - g0);   // rows of this tile inside the part
        unsigned sv = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
            if (row < nrow && topk_value(acc[r], w[r]) >= tv) sv |= 1u << r;
        }
        if (__any(sv != 0u)) {
            const int c0 = (int)(p.index_base + g0);                     // index_base + rows <= 2^31 - 1
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (sv & (1u << r)) {
                    const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
                    const unsigned long long key = search_pack(topk_key(acc[r], w[r], c0 + row), __float_as_uint(topk_value(acc[r], w[r])));
                    if (key > thr) pend[cnt++] = key;                    // cnt <= CL - 16 before the tile: room for all 16
                }
            }
            if (__any(cnt > CL - 16)) {                                  // a run that could not take another tile: wave-uniform
                search_compact_all(wbase, qstride, nslot, k, lane);
                thr = best[k - 1];                                       // both lanes of a query read its new k-th
                tv = thr ? search_key_value(thr) : -__builtin_inff();
                cnt = 0;
            }
        }
        if constexpr (PF) {
#pragma unroll
            for (int f = 0; f < NF; ++f) a[f] = an[f];
#pragma unroll
            for (int r = 0; r < 16; ++r) w[r] = wn[r];
        }
    }

    search_compact_all(wbase, qstride, nslot, k, lane);
    const int nlive = (int)min((long long)SEARCH_QW, p.nq - q0);
    for (int q = 0; q < nlive; ++q)
        if (lane < k)
            p.ws[((size_t)(q0 + q) * p.parts + blockIdx.y) * k + lane] = reinterpret_cast<const unsigned long long *>(wbase + (size_t)q * qstride)[lane];
}

template <bool PAIRS, int PER>
__global__ __launch_bounds__(256) void search_select_kernel(const unsigned long long *__restrict__ keys, const int *__restrict__ idx_in,
                                                            const float *__restrict__ val_in, int nq, long long n, int k,
                                                            int *__restrict__ idx, float *__restrict__ val) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= nq) return;                                                 // whole wavefronts leave: nothing below synchronises a block
    const size_t base = (size_t)b * n;
    auto key_at = [&](long long i) -> unsigned long long {
        if constexpr (PAIRS) {
            const float v = val_in[base + i];
            return search_pack(topk_key(1, v, idx_in[base + i]), __float_as_uint(v));          // fl32(1) * v == v
        } else {
            return keys[base + i];
        }
    };
    unsigned long long held[PER ? PER : 1];
    if constexpr (PER > 0) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const long long c = (long long)i * 64 + lane;
            held[i] = c < n ? key_at(c) : 0ull;
        }
    }
    unsigned long long last = ~0ull, mine = 0ull;
    for (int j = 0; j < k; ++j) {
        unsigned long long best = 0ull;
        if constexpr (PER > 0) {
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const unsigned long long cand = held[i] < last ? held[i] : 0ull;
                best = cand > best ? cand : best;
            }
        } else {
            for (long long i = lane; i < n; i += 64) {
                const unsigned long long key = key_at(i);
                const unsigned long long cand = key < last ? key : 0ull;
                best = cand > best ? cand : best;
            }
        }
        last = topk_wave_max(best);
        if (lane == j) mine = last;
    }
    if (lane < k) {
        idx[(size_t)b * k + lane] = search_key_index(mine);
        if (val) val[(size_t)b * k + lane] = search_key_value(mine);
    }
}

__global__ __launch_bounds__(256) void gallery_inv_norms_kernel(const int8_t *__restrict__ gallery, long long rows, int dim,
                                                                float *__restrict__ inv_norm) {
    const int sub = threadIdx.x & 15, nchunks = dim >> 4;
    // the 16 lanes of a row share g: they stay or leave together, and the sum below stays inside them
    for (long long g = (long long)blockIdx.x * 16 + (threadIdx.x >> 4); g < rows; g += (long long)gridDim.x * 16) {
        const v4i *row = reinterpret_cast<const v4i *>(gallery + (size_t)g * dim);
        int ss = 0;
        for (int c = sub; c < nchunks; c += 16) {
            const v4i v = row[c];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int b = 0; b < 4; ++b) { const int q = (int)(signed char)((unsigned)v[j] >> (8 * b)); ss += q * q; }
        }
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) ss += __shfl_xor(ss, d, 16);
        const double x = ss ? (double)ss : 1.0;
        double s = sqrt(x);
        s = fma(fma(-s, s, x), 0.5 / s, s);                              // the correctly rounded root (features_f32_kernel<UNIT>)
        if (sub == 0) inv_norm[g] = ss ? (float)(1.0 / s) : 0.0f;
    }
}
