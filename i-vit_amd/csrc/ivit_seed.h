// ivit_seed.h — k-means++ seeding on the device (include/ivit_seed.h): exact greedy D^2 sampling, one set-up launch and three launches
// per centre — scan, pick, locate — with the call's state (candidates, previous winner, stop flag) in the head of the workspace, so
// that no launch needs anything from the host.
//
//   d(r, j) = xx[r] - 2 dot[r, j] + xx[j]      mind[r] = the distance of row r to its nearest centre so far
//
// Workspace: SeedState (SEED_STATE_BYTES) | xx int32 [rows] | mind int32 [rows] | tab int64 [parts, 32]; a part is SEED_PART = 256 rows.
//
// seed_setup_kernel  xx[r] = sum_c x[r, c]^2 (16 lanes per row, as kmeans_norms_kernel) and mind[r] = SEED_INF; block 0 also writes
//   the state (every candidate = `first`, no previous winner, not stopped) and idx = -1, potential = 0, picked = K.  Step 0 is then an
//   ordinary step: all candidates equal, the lowest one wins, potential[0] = sum_r min(SEED_INF, d(r, first)).
//
// seed_scan_kernel<KS, PF>  the hot launch, dim = 64 KS: kmeans_assign_kernel (ivit_cluster.h) with the roles swapped.  One wavefront
//   per workgroup and per part.  The 32 candidate rows stay in 8 KS registers as the A operands of v_mfma_i32_32x32x32_i8 for the
//   whole launch (gathered through SeedState::cand; columns beyond `trials` repeat `first` and are never read back); the wavefront
//   walks its part 32 rows at a time as the B operand, so that after 2 KS MFMAs lane l holds, for row l % 32, the dot products with
//   candidates (r & 3) + 8 (r >> 2) + 4 (l / 32), r = 0 .. 15.
//   The previous winner is NOT a 33rd column.  mind in memory is lazy: it lacks the winner the pick chose after the last scan, so every
//   row needs d(r, previous winner) first.  As a column it would halve the tile at trials = 32 or need a second MFMA tile for one
//   useful column; instead the winner's bytes sit in 8 KS more registers in the operand layout and every lane takes its half of the
//   row's dot product with v_dot4_i32_i8 (4 KS instructions beside 2 KS MFMAs), the two halves meeting in one cross-lane move.
//   Per tile: mind' = min(mind, d(r, winner)) is stored back (lanes 0 .. 31), then every candidate's min(mind', d) is added into a
//   per-lane sum.  DEVIATION from int64 per-lane sums: a lane adds 8 values below 2^26 per candidate, so 32 bits hold them (2^29);
//   the sums widen to 64 bits in the cross-lane reduction at the end, where lanes 0 and 32 store the part's 32 sums with plain
//   vector stores.  Column w of tab is thereby the part sums of mind once w has won: the pick samples from it, no second pass.
//   xx comes from the once-computed array (4 bytes beside 64 KS per row), not from the row registers: 16 KS multiply-adds per tile
//   and lane saved.  Rows beyond the end: clamped on load, counted as 0, never stored.
//   Loads ahead of the MFMAs, the three regimes of kmeans_assign_kernel at its boundaries (registers from the -save-temps assembly in
//   DESIGN.md):
//     KS <= 7  (PF)   the next tile's 2 KS loads + xx + mind are issued, then this tile's MFMAs run with no wait among them
//     KS 8 .. 12      all loads of THIS tile are issued together, the MFMAs follow in order
//     KS 13 .. 16     the same in two halves of KS loads each; the winner's product takes a half's share before the next half is loaded
//   Each load phase ends in __builtin_amdgcn_sched_barrier(0) and a second one follows the MFMAs, as there.
//
// seed_pick_kernel  one workgroup: reduces tab per candidate, takes the lowest candidate of the smallest potential, writes idx, cent,
//   cnorm, potential and the state's previous winner; sets the stop flag and `picked` where the potential is 0; otherwise forms the
//   next step's t_l = __umul64hi(draw, total) and finds each one's part and residual in the winner's column: thread t sums a
//   contiguous run of parts, one block scan, and the thread whose run holds t_l walks it.
// seed_locate_kernel  one workgroup per next candidate, one thread per row of its part: min(mind, d(r, winner)) with v_dot4_i32_i8
//   against the winner's row in LDS, a block scan, and the one thread whose running sum first exceeds the residual stores its row.
// Every kernel returns at once when the stop flag is set.  Integers throughout; plain vector stores, no atomics, no scratch.
#pragma once
#include "../../include/ivit_seed.h"
#include "ivit_cluster.h"

#define SEED_MAX_TRIALS 32                         // candidates of a step: the M of the MFMA
#define SEED_TILES 8                               // 32-row tiles of a wavefront
#define SEED_PART (SEED_TILES * KMEANS_RW)         // rows of a part: one wavefront of the scan, one workgroup of the locate
#define SEED_INF 0x7fffffff                        // "no centre yet": above every distance
#define SEED_STATE_BYTES 1024
#define SEED_SETUP_MAX_BLOCKS (1 << 20)            // the set-up strides over the rows beyond that: its launch stays below 2^32 threads

struct SeedState {
    int cand[SEED_MAX_TRIALS];                     // rows of this step's candidates
    int part[SEED_MAX_TRIALS];                     // pick -> locate: the part that holds the next candidate l
    unsigned long long res[SEED_MAX_TRIALS];       // and what is left of t_l at the part's first row
    int prev;                                      // the last winner's row: the centre mind does not hold yet; -1 before step 0
    int stop;                                      // the potential reached 0: every later launch is a no-op
};
static_assert(sizeof(SeedState) <= SEED_STATE_BYTES, "the state fits the head of the workspace");
static_assert(SEED_PART == 256, "the locate kernel is one thread per row of a part");
static_assert(8ull * SEED_TILES * KMEANS_MAX_DIM * 255 * 255 < (1ull << 32), "a lane's 32-bit sums hold SEED_TILES distances");

struct SeedArgs {
    const int8_t *x;                    // [rows, dim]
    const unsigned long long *draws;    // [K, L]
    SeedState *st;
    int *xx, *mind;                     // [rows]
    unsigned long long *tab;            // [parts, 32]
    int8_t *cent;                       // [K, dim]
    int *cnorm, *idx;                   // [K]
    unsigned long long *potential;      // [K]
    int *picked;                        // [1]
    long long rows;
    int parts, dim, K, L, first;
};

__global__ __launch_bounds__(256) void seed_setup_kernel(SeedArgs p) {
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < p.K; i += 256) { p.idx[i] = -1; p.potential[i] = 0ull; }
        if (threadIdx.x < SEED_MAX_TRIALS) { p.st->cand[threadIdx.x] = p.first; p.st->part[threadIdx.x] = 0; p.st->res[threadIdx.x] = 0ull; }
        if (threadIdx.x == 0) { p.st->prev = -1; p.st->stop = 0; *p.picked = p.K; }
    }
    const int sub = threadIdx.x & 15, nchunks = p.dim >> 4;
    for (long long r = (long long)blockIdx.x * 16 + (threadIdx.x >> 4); r < p.rows; r += (long long)gridDim.x * 16) {
        const v4i *row = reinterpret_cast<const v4i *>(p.x + (size_t)r * p.dim);
        int ss = 0;
        for (int c = sub; c < nchunks; c += 16) {
            const v4i v = row[c];
#pragma unroll
            for (int i = 0; i < 4; ++i) ss = __builtin_amdgcn_sdot4(v[i], v[i], ss, false);
        }
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) ss += __shfl_xor(ss, d, 16);
        if (sub == 0) { p.xx[r] = ss; p.mind[r] = SEED_INF; }
    }
}

template <int KS, bool PF>
__global__ __launch_bounds__(64) void seed_scan_kernel(SeedArgs p) {
    constexpr int NF = 2 * KS, DIM = 64 * KS, PHASES = KS > KMEANS_WHOLE_MAX_KS ? 2 : 1, FP = NF / PHASES;
    if (p.st->stop) return;
    const int lane = threadIdx.x, half = lane >> 5, l31 = lane & 31;
    const long long r0 = (long long)blockIdx.x * SEED_PART;
    const int prev = p.st->prev;

    v4i cf[NF], wf[NF];                                                  // the candidates (A operands) and the previous winner, resident
    int bias[16];                                                        // the norms of the candidates this lane scores
    {
        const int8_t *src = p.x + (size_t)p.st->cand[l31] * DIM + 16 * half;
        const int8_t *win = p.x + (size_t)max(prev, 0) * DIM + 16 * half;
#pragma unroll
        for (int f = 0; f < NF; ++f) { cf[f] = *reinterpret_cast<const v4i *>(src + 32 * f); wf[f] = *reinterpret_cast<const v4i *>(win + 32 * f); }
#pragma unroll
        for (int r = 0; r < 16; ++r) bias[r] = p.xx[p.st->cand[(r & 3) + 8 * (r >> 2) + 4 * half]];
    }
    const int wn = p.xx[max(prev, 0)];

    // Loads only, nothing that waits for one: the k-steps [f0, f1) of tile t and, with f0 == 0, the row's sum of squares and its mind
    auto load_tile = [&](int t, int f0, int f1, v4i (&b)[NF], int &xxv, int &mv) {
        const long long rc = min(r0 + t * KMEANS_RW + l31, p.rows - 1);
        if (f0 == 0) { xxv = p.xx[rc]; mv = p.mind[rc]; }
        const int8_t *src = p.x + (size_t)rc * DIM + 16 * half;
#pragma unroll
        for (int f = f0; f < f1; ++f) b[f] = *reinterpret_cast<const v4i *>(src + 32 * f);
    };

    unsigned sum[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) sum[r] = 0u;
    v4i b[NF];
    int xxv = 0, mv = 0;
    if constexpr (PF) load_tile(0, 0, NF, b, xxv, mv);
#pragma unroll 1
    for (int t = 0; t < SEED_TILES; ++t) {
        v4i bn[PF ? NF : 1];
        int xxn = 0, mn = 0;
        v16i acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0;
        int dw = 0;                                                      // this lane's half of the row's product with the previous winner
        if constexpr (PF) {
            load_tile(t + 1, 0, NF, bn, xxn, mn);                        // clamped to the last row: always inside the arrays
            __builtin_amdgcn_sched_barrier(0);                           // the loads stay issued here (head comment)
#pragma unroll
            for (int f = 0; f < NF; ++f) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(cf[f], b[f], acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);                           // and the rotation, which waits for them, below
#pragma unroll
            for (int f = 0; f < NF; ++f)
#pragma unroll
                for (int c = 0; c < 4; ++c) dw = __builtin_amdgcn_sdot4(b[f][c], wf[f][c], dw, false);
        } else {
#pragma unroll
            for (int ph = 0; ph < PHASES; ++ph) {
                load_tile(t, ph * FP, (ph + 1) * FP, b, xxv, mv);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int f = ph * FP; f < (ph + 1) * FP; ++f) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(cf[f], b[f], acc, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);                       // the next phase's loads stay below
#pragma unroll
                for (int f = ph * FP; f < (ph + 1) * FP; ++f)            // the phase's share of the winner's product: its registers are free after it
#pragma unroll
                    for (int c = 0; c < 4; ++c) dw = __builtin_amdgcn_sdot4(b[f][c], wf[f][c], dw, false);
            }
        }
        dw += __shfl_xor(dw, 32, 64);
        const long long row = r0 + t * KMEANS_RW + l31;
        const bool valid = row < p.rows;
        const int d0 = prev >= 0 ? xxv - 2 * dw + wn : SEED_INF;
        const int m = valid ? min(mv, d0) : 0;                           // a row beyond the end adds 0 to every sum
        if (valid && half == 0 && prev >= 0) p.mind[row] = m;
#pragma unroll
        for (int r = 0; r < 16; ++r) sum[r] += (unsigned)min(m, xxv + bias[r] - 2 * acc[r]);
        if constexpr (PF) {
#pragma unroll
            for (int f = 0; f < NF; ++f) b[f] = bn[f];
            xxv = xxn; mv = mn;
        }
    }

#pragma unroll
    for (int r = 0; r < 16; ++r) {
        unsigned long long v = sum[r];
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);      // within the 32 lanes of a half
        if (l31 == 0) p.tab[(size_t)blockIdx.x * SEED_MAX_TRIALS + ((r & 3) + 8 * (r >> 2) + 4 * half)] = v;
    }
}

// inclusive sum over the 256 threads of a workgroup, in thread order; `wsum`: 4 words of LDS
__device__ __forceinline__ unsigned long long seed_block_scan(unsigned long long v, unsigned long long *wsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    for (int w = 0; w < wave; ++w) v += wsum[w];
    return v;
}

__global__ __launch_bounds__(256) void seed_pick_kernel(SeedArgs p, int s) {
    __shared__ unsigned long long red[8][SEED_MAX_TRIALS], pot[SEED_MAX_TRIALS], wsum[4];
    if (p.st->stop) return;
    const int t = threadIdx.x;
    {
        const int l = t & 31, g = t >> 5;                                // a table row is 256 contiguous bytes: 32 consecutive threads
        unsigned long long v = 0ull;
        for (int q = g; q < p.parts; q += 8) v += p.tab[(size_t)q * SEED_MAX_TRIALS + l];
        red[g][l] = v;
    }
    __syncthreads();
    if (t < SEED_MAX_TRIALS) {
        unsigned long long v = 0ull;
#pragma unroll
        for (int g = 0; g < 8; ++g) v += red[g][t];
        pot[t] = v;
    }
    __syncthreads();
    int w = 0;
    unsigned long long total = pot[0];
    for (int l = 1; l < p.L; ++l)
        if (pot[l] < total) { total = pot[l]; w = l; }                   // the lowest l of the smallest potential
    const int row = p.st->cand[w];
    {
        const int *src = reinterpret_cast<const int *>(p.x + (size_t)row * p.dim);
        int *dst = reinterpret_cast<int *>(p.cent + (size_t)s * p.dim);
        for (int i = t; i < (p.dim >> 2); i += 256) dst[i] = src[i];
    }
    __syncthreads();                                                     // every thread has read the state thread 0 now writes
    if (t == 0) { p.idx[s] = row; p.cnorm[s] = p.xx[row]; p.potential[s] = total; p.st->prev = row; }
    if (s + 1 >= p.K) return;
    if (total == 0ull) {                                                 // fewer distinct rows than K: s + 1 centres it is
        if (t == 0) { p.st->stop = 1; *p.picked = s + 1; }
        return;
    }
    const int chunk = (p.parts + 255) / 256, q0 = min(t * chunk, p.parts), q1 = min(q0 + chunk, p.parts);
    unsigned long long mine = 0ull;
    for (int q = q0; q < q1; ++q) mine += p.tab[(size_t)q * SEED_MAX_TRIALS + w];
    const unsigned long long below = seed_block_scan(mine, wsum) - mine;
    for (int l = 0; l < p.L; ++l) {
        const unsigned long long tl = __umul64hi(p.draws[(size_t)(s + 1) * p.L + l], total);    // < total
        if (tl < below || tl >= below + mine) continue;
        unsigned long long cum = below;
        for (int q = q0; q < q1; ++q) {
            const unsigned long long v = p.tab[(size_t)q * SEED_MAX_TRIALS + w];
            if (cum + v > tl) { p.st->part[l] = q; p.st->res[l] = tl - cum; break; }
            cum += v;
        }
    }
}

__global__ __launch_bounds__(256) void seed_locate_kernel(SeedArgs p, int s) {
    __shared__ int wrow[KMEANS_MAX_DIM / 4];
    __shared__ unsigned long long wsum[4];
    if (p.st->stop || s + 1 >= p.K) return;
    const int l = blockIdx.x, t = threadIdx.x, win = p.st->prev;
    const int part = min(max(p.st->part[l], 0), p.parts - 1);            // always a part of the table, whatever the state holds
    const unsigned long long res = p.st->res[l];
    for (int i = t; i < (p.dim >> 2); i += 256) wrow[i] = reinterpret_cast<const int *>(p.x + (size_t)win * p.dim)[i];
    __syncthreads();
    const long long row = (long long)part * SEED_PART + t;
    int m = 0;
    if (row < p.rows) {
        const v4i *src = reinterpret_cast<const v4i *>(p.x + (size_t)row * p.dim);
        int dot = 0;
        for (int c = 0; c < (p.dim >> 4); ++c) {
            const v4i v = src[c];
#pragma unroll
            for (int j = 0; j < 4; ++j) dot = __builtin_amdgcn_sdot4(v[j], wrow[4 * c + j], dot, false);
        }
        m = min(p.mind[row], p.xx[row] - 2 * dot + p.xx[win]);
    }
    const unsigned long long upto = seed_block_scan((unsigned long long)m, wsum);
    if (m > 0 && upto > res && upto - (unsigned long long)m <= res) p.st->cand[l] = (int)row;   // one thread at most
}
