// ivit_scan.h — the scan that gallery search, range search, density clustering, the linkage rounds and the core pass share, written
// once: a wavefront keeps 32 RESIDENT int8 rows (queries, or rows of the same array in a self-join) as the B operands of
// v_mfma_i32_32x32x32_i8 for the whole kernel and walks the other side 32 rows, a TILE, at a time.
//
//   work shape  a workgroup is four wavefronts that share nothing but the rows passing through the CU's vector cache; wavefront w of
//               block bx owns resident rows 128 bx + 32 w .. + 31 in 8 KS registers (dim = 64 KS, NF = 2 KS k-steps).
//   lanes       lane l holds bytes [32 f + 16 (l / 32), + 16) of row l % 32 for every k-step f: 16-byte loads, a tile's rows one
//               contiguous run.  After the NF MFMAs (scan_dot) lane l holds, for resident row l % 32, the 16 dot products of tile rows
//               scan_tile_row(r, l / 32), r = 0 .. 15, ascending in r.  The two lanes of a resident row are l and l ^ 32.
//   ends        rows beyond the end of either side are never loaded: every load is clamped to the last row (always inside the arrays);
//               scan_nrow says how many rows of a tile exist, `live` whether a lane's resident row exists.
//   prefetch    PF: the loads of the NEXT tile are issued before the MFMAs of this one, then rotated in (scan_rotate); off above
//               dim 512, where twice the tile does not fit beside the resident rows, and the tile is then loaded in place.
//   THE ORDER OF A TILE'S STEPS is part of the contract (seen on an MI355X, recorded in ivit_range.h): whatever decides which tile
//               comes next stands BEFORE the loads, and nothing that can become a branch stands between scan_dot and the first read
//               of its result.  With a branch there the compiler left one wait state before v_accvgpr_read of the last register,
//               which then still held the sum of the MFMA before.
// WHO USES WHAT.  The work shape, scan_tile_row, scan_nrow, scan_diag and scan_pair_value are used by all five kernels; scan_lane, the
// loads, scan_dot and scan_rotate by core_scan_kernel (ivit_hdbscan.h), the other four spell those steps out.  The loops stand in the
// kernels.  Measurements: profiles/README.md, "The shared scan".
#pragma once
#include "ivit_topk.h"

#define SEARCH_QW 32                               // resident rows of a wavefront: the N of the MFMA
#define SEARCH_QB (4 * SEARCH_QW)                  // resident rows of a workgroup
#define SEARCH_TILE 32                             // rows of a tile: the M of the MFMA
#define SEARCH_PF_MAX_KS 8                         // prefetch the next tile up to dim 512
__host__ __device__ constexpr bool scan_prefetch(int KS) { return KS <= SEARCH_PF_MAX_KS; }

// the tile row of accumulator register r in the lanes of `half`; with `base` the index of the tile's row 0, that row's index
template <class T = int>
__device__ __forceinline__ T scan_tile_row(int r, int half, T base = 0) { return base + (r & 3) + 8 * (r >> 2) + 4 * half; }

struct ScanLane {
    int lane, wave, half, l31;      // of the wavefront; of the workgroup; lane / 32; lane % 32
    long long q0;                   // the wavefront's first resident row: at or beyond `nres`, the whole wavefront has nothing to do
    long long qrow;                 // this lane's resident row, clamped to the last one: what the loads use
    bool live;                      // this lane's resident row exists
};
__device__ __forceinline__ ScanLane scan_lane(long long nres) {
    ScanLane s;
    s.lane = threadIdx.x & 63; s.wave = threadIdx.x >> 6; s.half = s.lane >> 5; s.l31 = s.lane & 31;
    s.q0 = ((long long)blockIdx.x * 4 + s.wave) * SEARCH_QW;
    s.qrow = min(s.q0 + s.l31, nres - 1);
    s.live = s.q0 + s.l31 < nres;
    return s;
}

// this lane's 16 bytes of every k-step of row `row` (inside the array): the resident rows once, a tile's rows per tile
template <int NF>
__device__ __forceinline__ void scan_load_rows(const int8_t *base, long long row, int half, v4i (&a)[NF]) {
    const int8_t *src = base + (size_t)row * (32 * NF) + 16 * half;
#pragma unroll
    for (int f = 0; f < NF; ++f) a[f] = *reinterpret_cast<const v4i *>(src + 32 * f);
}
// one float per accumulator register: weight[g0 + tile row], clamped to the last row; a null array is 1.0f throughout
__device__ __forceinline__ void scan_load_weights(const float *weight, long long g0, int half, long long last_row, float (&w)[16]) {
#pragma unroll
    for (int r = 0; r < 16; ++r) w[r] = weight ? weight[min(g0 + scan_tile_row(r, half), last_row)] : 1.0f;
}
// the tile that begins at row g0: its rows and their weights
template <int NF>
__device__ __forceinline__ void scan_load_tile(const int8_t *x, const float *weight, long long g0, const ScanLane &s, long long last_row, v4i (&a)[NF],
                                               float (&w)[16]) {
    scan_load_rows<NF>(x, min(g0 + s.l31, last_row), s.half, a);
    scan_load_weights(weight, g0, s.half, last_row, w);
}
// the prefetched registers become the current ones
template <class T, int N>
__device__ __forceinline__ void scan_rotate(T (&cur)[N], const T (&next)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) cur[i] = next[i];
}

// the 32 x 32 exact int32 products of a tile and the resident rows: read the result before anything that can branch
template <int NF>
__device__ __forceinline__ v16i scan_dot(const v4i (&a)[NF], const v4i (&qf)[NF]) {
    v16i acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0;
#pragma unroll
    for (int f = 0; f < NF; ++f) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[f], qf[f], acc, 0, 0, 0);
    return acc;
}

// rows of the tile at g0 that lie before `end`
__device__ __forceinline__ int scan_nrow(long long end, long long g0) { return (int)min((long long)SEARCH_TILE, end - g0); }
// the diagonal inside a tile: `d` is (the resident row's index) - (the index of the tile's row 0), and tile row `row` lies above the
// diagonal exactly when row > scan_diag(d); -1 lets every row pass
__device__ __forceinline__ int scan_diag(long long d) { return (int)max(-1ll, min((long long)SEARCH_TILE, d)); }

// THE VALUE OF A PAIR in a self-join (density clustering, the linkage rounds, the core pass: all three call this):
//   v{b, g} = fl32(fl32(fl32(dot) * weight[max(b, g)]) * weight[min(b, g)])
// first the weight of the LARGER row, then that of the smaller, chosen per element by `up` (the tile row lies above the resident
// row's diagonal: g > b): one value per unordered pair, whichever of the two is the resident row.  A null weight is two
// multiplications by 1.0f (the same bits).  DBSCAN's neighbours, the linkage tree and the core similarities agree with each other
// only while all three compute exactly this.
__device__ __forceinline__ float scan_pair_value(int acc, float w, float qw, bool up) {
    return __fmul_rn(topk_value(acc, up ? w : qw), up ? qw : w);
}
