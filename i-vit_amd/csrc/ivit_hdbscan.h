// ivit_hdbscan.h — the two device passes of HDBSCAN (include/ivit_hdbscan.h): a row's core similarity, the min_pts-th largest value of
// its row of the self-join, and the mutual-reachability round, which is linkage_scan_kernel<KS, PF, LINKAGE_REACH> of ivit_linkage.h and
// needs nothing here.  The scan and the value of a pair are those of ivit_scan.h (so that core[i] >= t exactly when
// ivit_density_degree counts min_pts rows at t), the candidate lists those of ivit_search.h on slots of CORE_SLOT bytes.
//
//   value   v{b, g} = scan_pair_value, counted as v + 0.0f.  A candidate is the 32-bit ordered value alone (topk_ordered of ivit_topk.h,
//           never 0 for a value that is not NaN): no index, nothing packed.  0 stands for "nothing".
//   core    the k-th largest element of the MULTISET { v{b, g} : g }, g == b included, equal values with their multiplicity.
//
// core_scan_kernel<KS, PF>  dim = 64 KS.  density_scan_kernel's grid, residents, tiles, prefetch and diagonal rule; every live row is
//   active.  Per wavefront 32 rows x (nslot + 1) 32-bit slots of LDS (nslot = 64: kcap 16, CL 24 for k <= 16; 128: kcap 64, CL 32 above;
//   the spare slot shifts the rows across the banks), half of search_scan_kernel's.  A row's threshold is the VALUE tv of its k-th
//   best so far, NaN until there is one, and the filter is STRICT, !(v <= tv): a value equal to the k-th cannot change the k-th
//   largest element of a multiset, so one compare is the whole test and no key is compared.  Survivors are appended to the lane's own
//   run (a row has two lanes; counts in registers, no atomics); when some run could not take another 16 the wavefront compacts all its
//   rows (search_compact_all<unsigned>: duplicates swap like anything else) and every lane takes its row's new
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

#define CORE_SLOT 4                                     // bytes of a candidate slot: search_nslot / _kcap / _qstride / _lds_bytes at this size

struct CoreArgs {
    const int8_t *x;                    // [rows, dim]
    const float *weight;                // [rows] or null
    unsigned *ws;                       // [rows, parts, k]
    float *core;                        // [rows]
    long long rows, tiles, per;         // part s covers tiles [s * per, min(tiles, (s + 1) * per))
    int k, parts;
};

template <int KS, bool PF>
__global__ __launch_bounds__(256) void core_scan_kernel(CoreArgs p) {
    constexpr int NF = 2 * KS;
    extern __shared__ __attribute__((aligned(16))) char core_sm[];
    const ScanLane s = scan_lane(p.rows);
    const int lane = s.lane, wave = s.wave, half = s.half, l31 = s.l31;
    const long long q0 = s.q0, qrow = s.qrow;
    if (q0 >= p.rows) return;                                            // whole wavefronts leave: nothing below synchronises a block
    const int k = p.k, nslot = search_nslot(k), kcap = search_kcap(k), CL = (nslot - kcap) >> 1, qstride = search_qstride(k, CORE_SLOT);
    char *wbase = core_sm + (size_t)wave * SEARCH_QW * qstride;
    for (int i = lane; i < SEARCH_QW * (nslot + 1); i += 64) reinterpret_cast<unsigned *>(wbase)[i] = 0u;
    const unsigned *best = reinterpret_cast<const unsigned *>(wbase + (size_t)l31 * qstride);              // this lane's row
    unsigned *pend = reinterpret_cast<unsigned *>(wbase + (size_t)l31 * qstride) + kcap + half * CL;       // this lane's run
    search_wave_sync();

    const bool live = s.live;                                            // this lane's row exists
    const long long last_row = p.rows - 1;
    const long long t_begin = (long long)blockIdx.y * p.per, t_end = min(p.tiles, t_begin + p.per);

    v4i qf[NF];
    scan_load_rows<NF>(p.x, qrow, half, qf);
    const float qw = p.weight ? p.weight[qrow] : 1.0f;

    float tv = __uint_as_float(0x7fc00000u);                             // NaN until the row has a k-th: !(v <= tv) holds for every v
    int cnt = 0;                                                         // values in this lane's run

    v4i a[NF];
    float w[16];
    if constexpr (PF) scan_load_tile<NF>(p.x, p.weight, t_begin * SEARCH_TILE, s, last_row, a, w);
    for (long long t = t_begin; t < t_end; ++t) {
        const long long g0 = t * SEARCH_TILE;
        v4i an[PF ? NF : 1];
        float wn[PF ? 16 : 1];
        // no next tile: this one again, from the cache
        if constexpr (PF) scan_load_tile<NF>(p.x, p.weight, min(t + 1, t_end - 1) * SEARCH_TILE, s, last_row, an, wn);
        else scan_load_tile<NF>(p.x, p.weight, g0, s, last_row, a, w);
        const v16i acc = scan_dot<NF>(a, qf);

        const int nrow = live ? scan_nrow(p.rows, g0) : 0;               // rows of this tile inside the array
        const int diag = scan_diag(q0 + l31 - g0);                       // tile row `row` is row g = g0 + row: g > b exactly when row > b - g0
        float v[16];
        unsigned sv = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = scan_tile_row(r, half);
            v[r] = scan_pair_value(acc[r], w[r], qw, row > diag) + 0.0f;
            if (row < nrow && !(v[r] <= tv)) sv |= 1u << r;
        }
        if (__any(sv != 0u)) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (sv & (1u << r)) pend[cnt++] = topk_ordered(v[r]);    // cnt <= CL - 16 before the tile: room for all 16
            if (__any(cnt > CL - 16)) {                                  // a run that could not take another tile: wave-uniform
                search_compact_all<unsigned>(wbase, qstride, nslot, k, lane);
                const unsigned thr = best[k - 1];                        // both lanes of a row read its new k-th
                tv = thr ? topk_ordered_value(thr) : __uint_as_float(0x7fc00000u);
                cnt = 0;
            }
        }
        if constexpr (PF) {
            scan_rotate(a, an);
            scan_rotate(w, wn);
        }
    }

    search_compact_all<unsigned>(wbase, qstride, nslot, k, lane);
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
    if (lane == 0) p.core[b] = topk_ordered_value(last);
}
