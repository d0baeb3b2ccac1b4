// ivit_kth.h — neighbour order statistics (include/ivit_kth.h): for every resident row (a query, or a row of the same array in a
// self-join) the k-th largest of its values against ALL rows of the other side, for any k up to the row count, by exact radix select.
// A candidate list (ivit_search.h, ivit_hdbscan.h) holds k values per row in LDS and cannot grow past 64; a histogram of one DIGIT of
// the value has the same size whatever k is.  The other side is streamed once per digit through the shared scan (ivit_scan.h) and the
// scores never leave registers.
//
//   key      u = topk_ordered(v + 0.0f) (ivit_topk.h): unsigned order == float order, -0.0 folded into +0.0.  Four digits of 8 bits, most
//            significant first: pass p = 0 .. 3 works on digit (u >> (24 - 8 p)) & 255.
//   state    per resident row a PREFIX (the digits chosen so far, in place, the bits below them 0), ABOVE (int64: values strictly
//            greater than every key under the prefix) and the pass.
//   count    in pass p a score counts exactly when its leading 8 p bits equal the prefix ((u & mask) == prefix, mask 0 in pass 0); it
//            increments its digit's bin.
//   pick     walk the bins from 255 down; the digit is the first bin at which above + cumulative >= k; above grows by the bins over it.
//            After pass 3 the prefix is the key: kth = topk_ordered_value(prefix), never -0.0, and above counts the values > kth.
//
// kth_scan_kernel<KS, PF, SELF>  dim = 64 KS.  The work shape, lanes, ends, prefetch and THE ORDER OF A TILE'S STEPS are ivit_scan.h's:
//   grid (128 resident rows) x (parts of the other side, whole tiles of 32).  SELF: the value is scan_pair_value (density clustering's,
//   the core pass's); otherwise ivit_range.h's, fl32(fl32(fl32(dot) * weight[g]) * qweight[b]).
//   histogram  per wavefront [32 resident rows][256] uint32 in dynamic LDS, a row's bins KTH_QSTRIDE = 257 words apart: 32 896 bytes a
//            wavefront, 131 584 a workgroup, one workgroup per CU.  That is why the digits have 8 bits: 11 / 11 / 10 would need 2048
//            bins a row.  The spare word matters in pass 0, where most scores of a wavefront share a sign and the top exponent bits
//            and so a bin: with a stride of 256 the 32 rows' copies of that bin lie in one bank, with 257 in 32 banks.
//   two lanes  of a resident row (l and l ^ 32) may hit the same bin in the same instruction.  CHOSEN: an LDS integer atomic add without
//            return (ds_add_u32), one LDS instruction per counted score, the hardware serialising equal addresses.  The alternative, an
//            exchange of the 16 digits between the lane pair and a merge of equal ones, is 16 cross-lane moves and as many compares per
//            tile before the same 16 LDS writes.  Integer counts have no order: the bits are the same either way.
//   skipping   from pass 1 on one ballot per tile skips the histogram step when no lane has a score under its prefix.
//   whole      parts == 1 (a wavefront's part is the whole other side; a self-join of many rows always gets it): the kernel runs all
//            four passes itself.  Between passes lane q < 32 walks row q's 256 bins in LDS and both lanes of a row take the new
//            prefix through one cross-lane read.  Only kth and above leave the CU: one launch, no workspace.
//   split      parts > 1: the kernel runs pass p.pass, reads the prefix where kth_pick_kernel left it, and stores its histograms to
//            hist[row][part][256] with plain stores.
// kth_pick_kernel  the split form's pick, one wavefront per resident row: lane l sums bins l, l + 64, l + 128, l + 192 over the parts in
//   int64, a suffix sum over the lanes per group of 64 bins and one ballot find the digit.  BETWEEN the passes the state lives in the
//   outputs themselves (the prefix as the bits of kth[b], above[b]); pass 3 leaves the results there.  Eight launches, no workgroup
//   waits for another.  Both forms add the same integers: the same bits.
// Plain vector stores only, no scratch.
#pragma once
#include "../../include/ivit_kth.h"
#include "ivit_search.h"

#define KTH_BINS 256
#define KTH_QSTRIDE (KTH_BINS + 1)                                   // words between two resident rows' histograms
#define KTH_LDS_BYTES (4 * SEARCH_QW * KTH_QSTRIDE * 4)              // four wavefronts

struct KthArgs {
    const int8_t *q;                    // [nq, dim]: the resident rows (x itself in a self-join)
    const int8_t *x;                    // [rows, dim]: the streamed side
    const float *weight;                // [rows] or null
    const float *qweight;               // [nq] or null; not read in a self-join
    unsigned *hist;                     // [nq, parts, 256]: the split form's workspace
    float *kth;                         // [nq]; between the split form's passes the prefix, as bits
    long long *above;                   // [nq]
    long long nq, rows, tiles, per;     // part s covers tiles [s * per, min(tiles, (s + 1) * per))
    long long k;
    int parts, pass;                    // pass: the digit a split-form launch works on
};

__device__ __forceinline__ int kth_shift(int pass) { return 24 - 8 * pass; }

template <int KS, bool PF, bool SELF>
__global__ __launch_bounds__(256) void kth_scan_kernel(KthArgs p) {
    constexpr int NF = 2 * KS;
    extern __shared__ __attribute__((aligned(16))) char kth_sm[];
    const ScanLane s = scan_lane(p.nq);
    const int lane = s.lane, half = s.half, l31 = s.l31;
    const long long q0 = s.q0;
    if (q0 >= p.nq) return;                                              // whole wavefronts leave: nothing below synchronises a block
    unsigned *hist = reinterpret_cast<unsigned *>(kth_sm) + (size_t)s.wave * SEARCH_QW * KTH_QSTRIDE;
    unsigned *mine = hist + l31 * KTH_QSTRIDE;                           // this lane's resident row
    const long long last_row = p.rows - 1;
    const long long t_begin = (long long)blockIdx.y * p.per, t_end = min(p.tiles, t_begin + p.per);
    const bool whole = p.parts == 1;

    v4i qf[NF];
    scan_load_rows<NF>(p.q, s.qrow, half, qf);
    const float qw = SELF ? (p.weight ? p.weight[s.qrow] : 1.0f) : (p.qweight ? p.qweight[s.qrow] : 1.0f);

    int pass = whole ? 0 : p.pass;
    unsigned prefix = pass ? reinterpret_cast<const unsigned *>(p.kth)[s.qrow] : 0u;
    long long above = 0;                                                 // the whole form's; the split form's stays in p.above
    for (;;) {
        const int shift = kth_shift(pass);
        const unsigned mask = pass ? 0xFFFFFFFFu << (shift + 8) : 0u;
        search_wave_sync();                                              // the walk of the pass before has read the bins
        for (int i = lane; i < SEARCH_QW * KTH_QSTRIDE; i += 64) hist[i] = 0u;
        search_wave_sync();

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

            const int nrow = s.live ? scan_nrow(p.rows, g0) : 0;         // rows of this tile inside the array
            const int diag = SELF ? scan_diag(q0 + l31 - g0) : 0;        // tile row `row` is row g = g0 + row: g > b exactly when row > b - g0
            unsigned u[16];
            unsigned under = 0u;                                         // scores of this lane under its prefix
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = scan_tile_row(r, half);
                const float v = SELF ? scan_pair_value(acc[r], w[r], qw, row > diag) : __fmul_rn(topk_value(acc[r], w[r]), qw);
                u[r] = topk_ordered(v + 0.0f);
                if (row < nrow && (u[r] & mask) == prefix) under |= 1u << r;
            }
            if (pass == 0 || __any(under != 0u)) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (under & (1u << r)) __hip_atomic_fetch_add(mine + ((u[r] >> shift) & 255u), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            if constexpr (PF) {
                scan_rotate(a, an);
                scan_rotate(w, wn);
            }
        }
        search_wave_sync();
        if (!whole) break;
        if (lane < SEARCH_QW) {                                          // lane q walks row q's bins (mine: l31 == lane)
            long long cum = 0;
            unsigned digit = 0u;
            for (int b = KTH_BINS - 1; b >= 0; --b) {
                const long long c = mine[b];
                if (above + cum + c >= p.k) { digit = (unsigned)b; break; }          // k <= rows: a live row always gets here
                cum += c;
            }
            above += cum;
            prefix |= digit << shift;
        }
        if (pass == 3) break;
        prefix = (unsigned)__shfl((int)prefix, l31);                     // the row's other lane
        ++pass;
    }

    if (whole) {
        if (lane < SEARCH_QW && s.live) {
            p.kth[q0 + lane] = topk_ordered_value(prefix);
            p.above[q0 + lane] = above;
        }
    } else {
        const int nlive = (int)min((long long)SEARCH_QW, p.nq - q0);
        for (int q = 0; q < nlive; ++q) {
            unsigned *dst = p.hist + ((size_t)(q0 + q) * p.parts + blockIdx.y) * KTH_BINS;
#pragma unroll
            for (int j = 0; j < KTH_BINS / 64; ++j) dst[64 * j + lane] = hist[q * KTH_QSTRIDE + 64 * j + lane];
        }
    }
}

__global__ __launch_bounds__(256) void kth_pick_kernel(KthArgs p) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= p.nq) return;                                               // whole wavefronts leave: nothing below synchronises a block
    const unsigned *src = p.hist + (size_t)b * p.parts * KTH_BINS;
    long long c[KTH_BINS / 64] = {};                                     // bins lane, lane + 64, ...: summed over the parts
    for (int part = 0; part < p.parts; ++part) {
#pragma unroll
        for (int j = 0; j < KTH_BINS / 64; ++j) c[j] += src[(size_t)part * KTH_BINS + 64 * j + lane];
    }
    unsigned prefix = p.pass ? reinterpret_cast<const unsigned *>(p.kth)[b] : 0u;
    long long above = p.pass ? p.above[b] : 0ll;
    long long over = 0, carry = 0;                                       // counts above the digit; counts of the groups above this one
    int digit = -1;                                                      // wave-uniform
#pragma unroll
    for (int j = KTH_BINS / 64 - 1; j >= 0; --j) {
        long long incl = c[j];                                           // this bin and the bins of the group above it
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long y = __shfl_down(incl, d, 64);
            if (lane + d < 64) incl += y;
        }
        const unsigned long long hit = __ballot(above + carry + incl >= p.k);        // monotone: every lane below a hit hits
        const int top = hit ? 63 - __clzll(hit) : 0;
        const long long over_here = carry + __shfl(incl - c[j], top, 64);
        if (digit < 0 && hit) {
            digit = 64 * j + top;
            over = over_here;
        }
        carry += __shfl(incl, 0, 64);
    }
    above += over;
    prefix |= (unsigned)max(digit, 0) << kth_shift(p.pass);              // k <= rows: some bin hits
    if (lane == 0) {
        if (p.pass == 3) p.kth[b] = topk_ordered_value(prefix);
        else reinterpret_cast<unsigned *>(p.kth)[b] = prefix;
        p.above[b] = above;
    }
}
