// ivit_hdbscan.h — the two device passes of HDBSCAN (include/ivit_hdbscan.h): a row's core similarity, the min_pts-th largest value of
// its row of the self-join, and the mutual-reachability round, which is linkage_scan_kernel<KS, PF, LINKAGE_REACH> of ivit_linkage.h and
// needs nothing here.  Takes from ivit_density.h the geometry of the scan and the value of a pair (so that core[i] >= t exactly when
// ivit_density_degree counts min_pts rows at t), from ivit_search.h the candidate lists, cut down to what a VALUE needs.
//
//   value   v{b, g} as csrc/ivit_density.h, counted as v + 0.0f.  A candidate is the 32-bit ordered value alone (core_key: topk_key's map,
//           unsigned order == float order, never 0 for a value that is not NaN): no index, nothing packed.  0 stands for "nothing".
//   core    the k-th largest element of the MULTISET { v{b, g} : g }, g == b included, equal values with their multiplicity.
//
// core_scan_kernel<KS, PF>  dim = 64 KS.  density_scan_kernel's grid, residents, tiles, prefetch and diagonal rule; every live row is
//   active.  Per wavefront 32 rows x (nslot + 1) 32-bit slots of LDS (nslot = 64: kcap 16, CL 24 for k <= 16; 128: kcap 64, CL 32 above;
//   the spare slot shifts the rows across the banks), half of search_scan_kernel's.  A row's threshold is the VALUE tv of its k-th
//   best so far, NaN until there is one, and the filter is STRICT, !(v <= tv): a value equal to the k-th cannot change the k-th
//   largest element of a multiset, so one compare is the whole test and no key is compared.  Survivors are appended to the lane's own
//   run (a row has two lanes; counts in registers, no atomics); when some run could not take another 16 the wavefront compacts all its
//   rows (core_compact_all: search_compact_all on 32-bit slots, duplicates swap like anything else) and every lane takes its row's new
//   tv from slot k - 1.  At the end of its part a wavefront compacts once more and lanes 0 .. k-1 store each row's k ordered values,
//   best first and 0-padded, to ws[(row * parts + part) * k ..].
// core_select_kernel<PER>   one wavefront per row over its n = parts * k ordered values, WITH multiplicity, a form of its own (the rounds
//   of search_select_kernel drop duplicates): round j takes the wave-wide maximum of the values below round j - 1's and the number of
//   slots that hold it (an integer sum over the wavefront) until k slots are covered — at most k rounds, fewer where values tie.  PER =
//   16: a lane holds slots l, l + 64, ... in registers (n <= 1024); PER = 0: every round rescans the slots from memory.  core[row] is
//   the inverse map of the last maximum: never -0.0.
// Plain vector stores only, no scratch.
#pragma once
#include "../../include/ivit_hdbscan.h"
#include "ivit_linkage.h"

#define CORE_MAX_K 64

__host__ __device__ __forceinline__ int core_nslot(int k) { return k <= 16 ? 64 : 128; }
__host__ __device__ __forceinline__ int core_kcap(int k) { return k <= 16 ? 16 : 64; }
// bytes between two rows' slots: one spare slot, so that the 32 rows of a wavefront start in different banks
__host__ __device__ __forceinline__ int core_qstride(int k) { return core_nslot(k) * 4 + 4; }
__host__ __device__ __forceinline__ size_t core_lds_bytes(int k) { return (size_t)SEARCH_QB * core_qstride(k); }

__device__ __forceinline__ unsigned core_key(float v) {
    unsigned u = __float_as_uint(v);
    u = u == 0x80000000u ? 0u : u;                                       // topk_key's map of a value
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float core_key_value(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

struct CoreArgs {
    const int8_t *x;                    // [rows, dim]
    const float *weight;                // [rows] or null
    unsigned *ws;                       // [rows, parts, k]
    float *core;                        // [rows]
    long long rows, tiles, per;         // part s covers tiles [s * per, min(tiles, (s + 1) * per))
    int k, parts;
};

// search_compact_all on 32-bit slots: lane q < 32 alone sorts the k best of row q's nslot slots to the front and zeroes the rest
__device__ __forceinline__ void core_compact_all(char *wbase, int qstride, int nslot, int k, int lane) {
    search_wave_sync();
    if (lane < SEARCH_QW) {
        unsigned *s = reinterpret_cast<unsigned *>(wbase + (size_t)lane * qstride);
        for (int j = 0; j < k; ++j) {
            unsigned best = s[j];
            int pos = j;
#pragma unroll 8
            for (int i = j + 1; i < nslot; ++i) {
                const unsigned e = s[i];
                if (e > best) { best = e; pos = i; }
            }
            if (best == 0u) break;                                       // nothing is left: the rest is zeros already
            const unsigned t = s[j];
            s[pos] = t;
            s[j] = best;
        }
        for (int i = k; i < nslot; ++i) s[i] = 0u;
    }
    search_wave_sync();
}

template <int KS, bool PF>
__global__ __launch_bounds__(256) void core_scan_kernel(CoreArgs p) {
    constexpr int NF = 2 * KS, DIM = 64 * KS;
    extern __shared__ __attribute__((aligned(16))) char core_sm[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const long long q0 = ((long long)blockIdx.x * 4 + wave) * SEARCH_QW;
    if (q0 >= p.rows) return;                                            // whole wavefronts leave: nothing below synchronises a block
    const int k = p.k, nslot = core_nslot(k), kcap = core_kcap(k), CL = (nslot - kcap) >> 1, qstride = core_qstride(k);
    char *wbase = core_sm + (size_t)wave * SEARCH_QW * qstride;
    for (int i = lane; i < SEARCH_QW * (nslot + 1); i += 64) reinterpret_cast<unsigned *>(wbase)[i] = 0u;
    const unsigned *best = reinterpret_cast<const unsigned *>(wbase + (size_t)l31 * qstride);              // this lane's row
    unsigned *pend = reinterpret_cast<unsigned *>(wbase + (size_t)l31 * qstride) + kcap + half * CL;       // this lane's run
    search_wave_sync();

    const bool live = q0 + l31 < p.rows;                                 // this lane's row exists
    const long long last_row = p.rows - 1;
    const long long qrow = min(q0 + l31, last_row);
    const long long t_begin = (long long)blockIdx.y * p.per, t_end = min(p.tiles, t_begin + p.per);

    v4i qf[NF];
    {
        const int8_t *src = p.x + (size_t)qrow * DIM + 16 * half;
#pragma unroll
        for (int f = 0; f < NF; ++f) qf[f] = *reinterpret_cast<const v4i *>(src + 32 * f);
    }
    const float qw = p.weight ? p.weight[qrow] : 1.0f;
    auto load_tile = [&](long long g0, v4i (&a)[NF], float (&w)[16]) {
        const int8_t *src = p.x + (size_t)min(g0 + l31, last_row) * DIM + 16 * half;
#pragma unroll
        for (int f = 0; f < NF; ++f) a[f] = *reinterpret_cast<const v4i *>(src + 32 * f);
#pragma unroll
        for (int r = 0; r < 16; ++r) w[r] = p.weight ? p.weight[min(g0 + ((r & 3) + 8 * (r >> 2) + 4 * half), last_row)] : 1.0f;
    };

    float tv = __uint_as_float(0x7fc00000u);                             // NaN until the row has a k-th: !(v <= tv) holds for every v
    int cnt = 0;                                                         // values in this lane's run

    v4i a[NF];
    float w[16];
    if constexpr (PF) load_tile(t_begin * SEARCH_TILE, a, w);
    for (long long t = t_begin; t < t_end; ++t) {
        const long long g0 = t * SEARCH_TILE;
        v4i an[PF ? NF : 1];
        float wn[PF ? 16 : 1];
        if constexpr (PF) load_tile(min(t + 1, t_end - 1) * SEARCH_TILE, an, wn);             // no next tile: this one again, from the cache
        else load_tile(g0, a, w);
        v16i acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0;
#pragma unroll
        for (int f = 0; f < NF; ++f) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[f], qf[f], acc, 0, 0, 0);

        const int nrow = live ? (int)min((long long)SEARCH_TILE, p.rows - g0) : 0;            // rows of this tile inside the array
        // tile row `row` is row g = g0 + row of the array: g > b exactly when row > b - g0
        const int diag = (int)max(-1ll, min((long long)SEARCH_TILE, q0 + l31 - g0));
        float v[16];
        unsigned sv = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
            const bool up = row > diag;                                  // the larger row's weight first
            v[r] = __fmul_rn(topk_value(acc[r], up ? w[r] : qw), up ? qw : w[r]) + 0.0f;
            if (row < nrow && !(v[r] <= tv)) sv |= 1u << r;
        }
        if (__any(sv != 0u)) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (sv & (1u << r)) pend[cnt++] = core_key(v[r]);        // cnt <= CL - 16 before the tile: room for all 16
            if (__any(cnt > CL - 16)) {                                  // a run that could not take another tile: wave-uniform
                core_compact_all(wbase, qstride, nslot, k, lane);
                const unsigned thr = best[k - 1];                        // both lanes of a row read its new k-th
                tv = thr ? core_key_value(thr) : __uint_as_float(0x7fc00000u);
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

    core_compact_all(wbase, qstride, nslot, k, lane);
    const int nlive = (int)min((long long)SEARCH_QW, p.rows - q0);
    for (int q = 0; q < nlive; ++q)
        if (lane < k) p.ws[((size_t)(q0 + q) * p.parts + blockIdx.y) * k + lane] = reinterpret_cast<const unsigned *>(wbase + (size_t)q * qstride)[lane];
}

template <int PER>
__global__ __launch_bounds__(256) void core_select_kernel(CoreArgs p) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= p.rows) return;                                             // whole wavefronts leave: nothing below synchronises a block
    const long long n = (long long)p.parts * p.k;
    const unsigned *src = p.ws + (size_t)b * n;
    unsigned held[PER ? PER : 1];
    if constexpr (PER > 0) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const long long c = (long long)i * 64 + lane;
            held[i] = c < n ? src[c] : 0u;
        }
    }
    unsigned last = 0xFFFFFFFFu;                                         // above every ordered value of a finite float
    int covered = 0;                                                     // slots at or above `last`: wave-uniform
    while (covered < p.k) {
        unsigned best = 0u;
        if constexpr (PER > 0) {
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const unsigned cand = held[i] < last ? held[i] : 0u;
                best = cand > best ? cand : best;
            }
        } else {
            for (long long i = lane; i < n; i += 64) {
                const unsigned cand = src[i] < last ? src[i] : 0u;
                best = cand > best ? cand : best;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned o = __shfl_xor(best, d, 64);
            best = o > best ? o : best;
        }
        if (best == 0u) break;                                           // fewer than k values: k <= rows rules it out
        int same = 0;
        if constexpr (PER > 0) {
#pragma unroll
            for (int i = 0; i < PER; ++i) same += held[i] == best;
        } else {
            for (long long i = lane; i < n; i += 64) same += src[i] == best;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) same += __shfl_xor(same, d, 64);
        covered += same;
        last = best;
    }
    if (lane == 0) p.core[b] = core_key_value(last);
}
