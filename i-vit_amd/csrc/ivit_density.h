// ivit_density.h — density clustering (include/ivit_density.h): DBSCAN over int8 rows as label propagation, the adjacency never
// written.  Per row only the NUMBER of its neighbours (the degree pass) or the SMALLEST LABEL among them (a sweep, the border pass) is
// needed, and a scan that keeps the scores in registers produces either directly.  The work shape, the lane layout of a tile
// (scan_tile_row), its bounds and the value of a pair are those of ivit_scan.h.
//
//   value      v{b, g} = scan_pair_value of ivit_scan.h, defined there: one value per unordered pair.
//   neighbour  v >= threshold (the IEEE comparison), g == b included.
//
// density_scan_kernel<KS, PF, MODE>  dim = 64 KS; ONE source for the three passes, so that they cannot disagree about a neighbour.
//   Grid (tiles of 128 resident rows) x (parts of the same rows, each a run of whole 32-row tiles: a dirty bit has one meaning); four
//   wavefronts per workgroup that share nothing but the rows passing through the CU's vector cache.  Wavefront w keeps rows 128 bx +
//   32 w .. + 31 as the B operands of v_mfma_i32_32x32x32_i8 and walks the tiles of its part; after 2 KS MFMAs lane l holds, for
//   resident row l % 32, the 16 dot products of tile rows (r & 3) + 8 (r >> 2) + 4 (l / 32), r = 0 .. 15, and builds a 16-bit mask
//   of its neighbours.
//   The walk: the part's tiles are the set bits of a 64-bit word at a time — the words of dirty_in in a sweep, all ones otherwise —
//   masked to the part, taken with count-trailing-zeros: wave-uniform scalar work.  A tile whose bit is clear costs neither its
//   loads nor its MFMAs, and the prefetch (PF; off above dim 512) targets the NEXT SET BIT.  The search for it stands BEFORE the
//   loads: no branch between a tile's last MFMA and the reads of its accumulators (the warning in ivit_range.h).
//   MODE  DENSITY_DEGREE  every row is active; a lane counts its neighbours.
//         DENSITY_SWEEP   active: core rows (label[q] != DENSITY_NONE).  A lane starts at label[q] and takes the minimum with
//                         label[g] of every neighbour g; a neighbour that is not core holds DENSITY_NONE, which makes the core test
//                         free.  Labels are gathered only for rows that hit, and only in tiles with a hit.
//         DENSITY_BORDER  active: the rows that are NOT core; a lane starts at DENSITY_NONE, the same minimum.
//   A wavefront none of whose 32 rows is active skips the walk.  Every wavefront, that one too, ends alike: ONE exchange with lane
//   l ^ 32 combines the two lanes of a row (sum or minimum), lanes 0 .. 31 store part[row * parts + part], ONE plain store per (row,
//   part): every element of `part` is written by every launch.  Rows beyond the end: the loads are clamped to the last row, such a
//   row is never counted, gathered or stored.  No LDS, no atomics, no scratch.
//
// density_fold_kernel<MODE>   a thread per row: the sum (degree) or minimum of its parts -> degree / m; border mode: a core row's
//                             label is copied, DENSITY_NONE becomes -1.
// density_jump_kernel         a thread per row: label_out[q] = m[m[q]] for a core row (a value that is no row is not followed),
//                             DENSITY_NONE otherwise; one ballot per wavefront gives the changed byte of its two tiles.
// density_pack_kernel         ONE workgroup: 64 bytes -> one word of dirty_out, the words' population counts -> changed.
// density_init_kernel         a workgroup per word of the bitmap (2048 rows): label = row or DENSITY_NONE, the tiles' ballots -> dirty.
// Plain vector stores only.
#pragma once
#include "../../include/ivit_density.h"
#include "ivit_search.h"

#define DENSITY_NONE 0x7fffffff                        // the label of a row that is not core
#define DENSITY_DEGREE 0
#define DENSITY_SWEEP 1
#define DENSITY_BORDER 2
#define DENSITY_WORD_TILES 64                          // tiles of a bitmap word
#define DENSITY_WORD_ROWS (DENSITY_WORD_TILES * SEARCH_TILE)

struct DensityArgs {
    const int8_t *x;                    // [rows, dim]
    const float *weight;                // [rows] or null
    const int *label;                   // [rows]: sweep and border
    const unsigned long long *dirty;    // [words]: sweep
    int *part;                          // [rows, parts]
    long long rows, tiles, per;         // part s covers tiles [s * per, min(tiles, (s + 1) * per))
    float threshold;
    int parts;
};

template <int KS, bool PF, int MODE>
__global__ __launch_bounds__(256) void density_scan_kernel(DensityArgs p) {
    constexpr int NF = 2 * KS, DIM = 64 * KS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const long long q0 = ((long long)blockIdx.x * 4 + wave) * SEARCH_QW;
    if (q0 >= p.rows) return;                                            // whole wavefronts leave: nothing below synchronises a block
    const bool live = q0 + l31 < p.rows;                                 // this lane's row exists
    const long long last_row = p.rows - 1;
    const long long qrow = min(q0 + l31, last_row);

    int best = MODE == DENSITY_DEGREE ? 0 : DENSITY_NONE;                // the count, or the running minimum
    bool active = live;
    if constexpr (MODE != DENSITY_DEGREE) {
        const int mine = p.label[qrow];
        active = live && (MODE == DENSITY_SWEEP ? mine != DENSITY_NONE : mine == DENSITY_NONE);
        if (MODE == DENSITY_SWEEP && active) best = mine;
    }

    if (__any(active)) {
        // the tiles of the part, a word of 64 at a time: wave-uniform
        const long long t_begin = (long long)blockIdx.y * p.per, t_end = min(p.tiles, t_begin + p.per);
        const long long w_first = t_begin >> 6, w_last = (t_end - 1) >> 6;
        auto word = [&](long long i) -> unsigned long long {
            unsigned long long b = ~0ull;
            if constexpr (MODE == DENSITY_SWEEP) b = p.dirty[i];
            if (i == w_first) b &= ~0ull << (t_begin & 63);
            if (i == w_last && (t_end & 63)) b &= ~0ull >> (64 - (t_end & 63));
            return b;
        };
        long long wi = w_first;
        unsigned long long cur = t_begin < t_end ? word(wi) : 0ull;
        auto next_tile = [&]() -> long long {                            // the next set bit, or -1
            while (cur == 0ull) {
                if (++wi > w_last) return -1;
                cur = word(wi);
            }
            const int b = __builtin_ctzll(cur);
            cur &= cur - 1ull;
            return wi * DENSITY_WORD_TILES + b;
        };

        v4i qf[NF];
        {
            const int8_t *src = p.x + (size_t)qrow * DIM + 16 * half;
#pragma unroll
            for (int f = 0; f < NF; ++f) qf[f] = *reinterpret_cast<const v4i *>(src + 32 * f);
        }
        const float qw = p.weight ? p.weight[qrow] : 1.0f;
        const float thr = p.threshold;
        auto load_tile = [&](long long g0, v4i (&a)[NF], float (&w)[16]) {
            const int8_t *src = p.x + (size_t)min(g0 + l31, last_row) * DIM + 16 * half;
#pragma unroll
            for (int f = 0; f < NF; ++f) a[f] = *reinterpret_cast<const v4i *>(src + 32 * f);
#pragma unroll
            for (int r = 0; r < 16; ++r) w[r] = p.weight ? p.weight[min(g0 + scan_tile_row(r, half), last_row)] : 1.0f;
        };

        long long t = next_tile();
        if (t >= 0) {
            v4i a[NF];
            float w[16];
            if constexpr (PF) load_tile(t * SEARCH_TILE, a, w);
            do {
                const long long tn = next_tile();                        // the branches of the search: before the loads
                const long long g0 = t * SEARCH_TILE;
                v4i an[PF ? NF : 1];
                float wn[PF ? 16 : 1];
                if constexpr (PF) load_tile((tn >= 0 ? tn : t) * SEARCH_TILE, an, wn);       // no next tile: this one again, from the cache
                else load_tile(g0, a, w);
                v16i acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0;
#pragma unroll
                for (int f = 0; f < NF; ++f) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[f], qf[f], acc, 0, 0, 0);

                const int nrow = active ? scan_nrow(p.rows, g0) : 0; // rows of this tile inside the array
                // tile row `row` is row g = g0 + row of the array: g > b exactly when row > b - g0
                const int diag = scan_diag(q0 + l31 - g0);
                unsigned mask = 0u;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = scan_tile_row(r, half);
                    const bool up = row > diag;                          // the larger row's weight first
                    const float v = scan_pair_value(acc[r], w[r], qw, up);
                    if (row < nrow && v >= thr) mask |= 1u << r;
                }
                if (__any(mask != 0u)) {
                    if constexpr (MODE == DENSITY_DEGREE) {
                        best += __popc(mask);
                    } else {
#pragma unroll
                        for (int r = 0; r < 16; ++r)                      // row < nrow: inside the array.  scan_tile_row(r, half, g0) written out:
                            // through the call the sweep and border passes allocate differently (one register more at dim 832)
                            if (mask & (1u << r)) best = min(best, p.label[g0 + (r & 3) + 8 * (r >> 2) + 4 * half]);
                    }
                }
                if constexpr (PF) {
#pragma unroll
                    for (int f = 0; f < NF; ++f) a[f] = an[f];
#pragma unroll
                    for (int r = 0; r < 16; ++r) w[r] = wn[r];
                }
                t = tn;
            } while (t >= 0);
        }
    }

    const int other = __shfl_xor(best, 32);                              // the two lanes of a row; every lane of the wavefront is here
    best = MODE == DENSITY_DEGREE ? best + other : min(best, other);
    if (half == 0 && live) p.part[(size_t)(q0 + l31) * p.parts + blockIdx.y] = best;
}

struct DensityFoldArgs {
    const int *part;        // [rows, parts]
    const int *label;       // [rows]: border
    int *out;               // [rows]: degree, m or out
    long long rows;
    int parts;
};

template <int MODE>
__global__ __launch_bounds__(256) void density_fold_kernel(DensityFoldArgs p) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= p.rows) return;
    const int *src = p.part + (size_t)q * p.parts;
    int r = src[0];
    for (int s = 1; s < p.parts; ++s) r = MODE == DENSITY_DEGREE ? r + src[s] : min(r, src[s]);
    if constexpr (MODE == DENSITY_BORDER) {
        const int mine = p.label[q];
        r = mine != DENSITY_NONE ? mine : (r == DENSITY_NONE ? -1 : r);
    }
    p.out[q] = r;
}

__global__ __launch_bounds__(256) void density_jump_kernel(const int *__restrict__ m, const int *__restrict__ label_in, int *__restrict__ label_out,
                                                           unsigned char *__restrict__ flag, long long rows, long long tiles) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    bool changed = false;
    if (q < rows) {
        const int before = label_in[q];
        int after = DENSITY_NONE;
        if (before != DENSITY_NONE) {
            after = m[q];
            if ((unsigned long long)(long long)after < (unsigned long long)rows) after = min(after, m[after]);      // only a row is followed
        }
        label_out[q] = after;
        changed = after != before;
    }
    const unsigned long long b = __ballot(changed);                      // a wavefront is two tiles
    const int lane = threadIdx.x & 63;
    const long long tile = q >> 5;
    if ((lane & 31) == 0 && tile < tiles) flag[tile] = (unsigned char)(((b >> lane) & 0xffffffffull) != 0ull);
}

// `flag` holds whole words of 64 bytes (the workspace pads it); what stands behind the last tile is masked, not read as a tile
__global__ __launch_bounds__(256) void density_pack_kernel(const unsigned char *__restrict__ flag, long long tiles, unsigned long long *__restrict__ dirty,
                                                           int *__restrict__ changed) {
    __shared__ int wave_sum[4];
    const long long words = (tiles + DENSITY_WORD_TILES - 1) / DENSITY_WORD_TILES;
    int count = 0;
    for (long long w = threadIdx.x; w < words; w += 256) {
        const v4i *src = reinterpret_cast<const v4i *>(flag + w * DENSITY_WORD_TILES);
        unsigned long long bits = 0ull;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const v4i x = src[i];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const unsigned u = (unsigned)x[c];                       // four bytes of 0 / 1 -> four bits
                const unsigned nib = (u & 1u) | ((u >> 7) & 2u) | ((u >> 14) & 4u) | ((u >> 21) & 8u);
                bits |= (unsigned long long)nib << (16 * i + 4 * c);
            }
        }
        const long long left = tiles - w * DENSITY_WORD_TILES;
        if (left < DENSITY_WORD_TILES) bits &= (1ull << left) - 1ull;
        dirty[w] = bits;
        count += __popcll(bits);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) count += __shfl_xor(count, d);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) *changed = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
}

__global__ __launch_bounds__(256) void density_init_kernel(const int *__restrict__ degree, long long rows, int min_pts, int *__restrict__ label,
                                                           unsigned long long *__restrict__ dirty) {
    __shared__ unsigned long long wave_bits[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * DENSITY_WORD_ROWS;
    unsigned long long bits = 0ull;
#pragma unroll
    for (int i = 0; i < DENSITY_WORD_ROWS / 256; ++i) {
        const long long q = base + i * 256 + threadIdx.x;
        bool core = false;
        if (q < rows) {
            core = degree[q] >= min_pts;
            label[q] = core ? (int)q : DENSITY_NONE;
        }
        const unsigned long long b = __ballot(core);                     // tiles 8 i + 2 wave and + 1 of the word
        bits |= (unsigned long long)((b & 0xffffffffull) != 0ull) << (8 * i + 2 * wave);
        bits |= (unsigned long long)((b >> 32) != 0ull) << (8 * i + 2 * wave + 1);
    }
    if (lane == 0) wave_bits[wave] = bits;
    __syncthreads();
    if (threadIdx.x == 0) dirty[blockIdx.x] = wave_bits[0] | wave_bits[1] | wave_bits[2] | wave_bits[3];
}
