// ivit_linkage.h — the single-linkage hierarchy (include/ivit_linkage.h): the maximum-similarity spanning forest of int8 rows by
// Borůvka rounds, the [rows, rows] matrix never written.  Per round every row needs ONE thing from a pass over all rows: its best
// neighbour outside its own component, and a scan that keeps the scores in registers produces it directly.  Takes from ivit_search.h
// the work shape (SEARCH_QW, SEARCH_QB, SEARCH_TILE, SEARCH_PF_MAX_KS: ivit_scan.h), from ivit_topk.h topk_value, the key of a value
// and the inverse of the ordered value, from ivit_scan.h the geometry of the scan and the value of a pair (scan_pair_value).
//
//   value      v{b, g} = scan_pair_value of ivit_scan.h: one value per unordered pair, whichever of the two is the resident row.
//   edge order v descending (-0.0 equal to +0.0), then the smaller row ascending, then the larger row ascending: total.
//   FOR A FIXED ROW q the order of its edges {q, g} is "largest v, then smallest g".  Among edges of equal v those with g < q have the
//              smaller row g < q and stand before every edge with g > q (smaller row q); among the former the smaller row IS g, among
//              the latter the smaller row is q for all and the larger row IS g.  Both runs ascend in g and the first lies below the
//              second: ascending g throughout.  A row's best edge is therefore one 64-bit key, topk_key(v, g) = topk_ordered(v) << 32 |
//              0xFFFFFFFF - g, and the larger key is the better edge; topk_ordered is ivit_topk.h's map (unsigned order == float order, -0.0
//              folded into +0.0), never 0 for a value that is not NaN, so key 0 is "no edge".
//
// linkage_scan_kernel<KS, PF, MODE>   dim = 64 KS; ONE source for the plain round and the mutual-reachability round below.  Grid (tiles of 128 resident rows) x (parts of the same rows, whole tiles of 32); four
//   wavefronts per workgroup that share nothing.  Wavefront w keeps rows 128 bx + 32 w .. + 31 as the B operands of
//   v_mfma_i32_32x32x32_i8 and walks the tiles of its part in ascending order; after 2 KS MFMAs lane l holds, for resident row l % 32,
//   the 16 values of tile rows (r & 3) + 8 (r >> 2) + 4 (l / 32), ascending in r.  A lane keeps ONE running best (value, g), NaN / -1
//   for none.  Because the walk ascends in g, a later row replaces the best only with a STRICTLY larger value: one compare, !(v <=
//   best), true against the NaN of "none", rejects the rest — and with v >= floor it is the whole test of a tile.  Only in a tile where
//   some lane holds a survivor are component ids gathered, for the survivors alone, and a survivor of another component becomes the
//   best.  The prefetch (PF; off above dim 512) loads the next tile, clamped to the last row.
//   A row is active when it exists and its component is not done; a wavefront without an active row skips the walk, and when
//   state.merged == 0 on entry (the forest is complete) every wavefront leaves at once, nothing written.  Otherwise every wavefront
//   ends alike: ONE exchange with lane l ^ 32 combines the two lanes of a row (the larger key), lanes 0 .. 31 store part[row * parts +
//   part], ONE plain store per (row, part); the wavefronts of part 0 also reset their rows' entries of cbest / cedge and the first
//   of them the hook counter, which the later launches of the round fill.  No LDS, no scratch; no atomics in the scan.
//   MODE  LINKAGE_PLAIN  the edge value is v (include/ivit_linkage.h).
//         LINKAGE_REACH  the edge value is m{q, g} = min(v, core[q], core[g]) (include/ivit_hdbscan.h), v counted as v + 0.0f.  The tile
//                        rows' core values travel with their weights (prefetched with them where PFC is on), the resident row's cq is
//                        loaded once.  v is an upper bound of m: the compare of a tile stays !(v <= best) and v >= floor on v, and only
//                        a survivor pays the two minimums, the floor test on m and the compare of m.  THE SATURATION EXIT: m{q, .} <=
//                        cq and the walk ascends in g, so a row one of whose two lanes holds best == cq at the end of a tile has its
//                        final edge of this part; one ballot per tile, its two halves ORed, against the active rows' mask, and the
//                        wavefront leaves the walk when every active row is settled.
//
// linkage_fold_kernel     a thread per row: the largest key of its parts -> rbest[row]; its ordered value goes into cbest[comp[row]]
//                         with an integer atomicMax (skipped where a relaxed read shows it is already there: the value only grows).
// linkage_pick_kernel     a thread per row: a row whose value attains cbest of its component offers min(q, g) << 32 | max(q, g) to
//                         cedge[comp[row]] with an integer atomicMin.  After the two passes (cbest, cedge) is the component's best edge
//                         under the full edge order.  Maximum and minimum of integers: the bits do not depend on the scheduling.
//                         THE ATOMIC FORM of the issue's two, in plain HIP C++ on global memory.
// linkage_hook_kernel     a thread per row c that is a component id (comp[c] == c) and not done: no edge -> done[c] = 1 (its outgoing
//                         edges can never change: exact); otherwise the edge's far end lies in component d = comp[far], and c hooks
//                         below d — parent[c] = d, the edge written into slot c — unless d chose the same edge and c < d (then c stays
//                         the root).  Distinct best edges under a total order admit no longer cycle.  A component that hooks stops
//                         existing, so slot c is written at most once in a run.  The hooks are counted with one atomicAdd of a
//                         ballot's population count per wavefront: an integer sum.
// linkage_jump_kernel     a thread per row: comp[q] follows parent to its root, a LOOP OVER THE READ-ONLY parent ARRAY (the launch
//                         count does not depend on the data).  Its worst case is the longest chain of hooks of the round, at most
//                         components - 1 steps (a path of components each of which chose the next); the chains of shuffled path graphs
//                         in the tests are a handful of steps.
// linkage_finish_kernel   ONE thread: components -= hooks, merged = hooks, rounds += 1 where anything hooked.
// linkage_init_kernel     a thread per row: comp, done, the edge slots; thread 0 the state.
// Every launch of a round but the scan leaves at once, too, when state.merged == 0 on entry.  Plain vector stores only.
#pragma once
#include "../../include/ivit_linkage.h"
#include "ivit_search.h"

struct LinkageArgs {
    const int8_t *x;                    // [rows, dim]
    const float *weight;                // [rows] or null
    int *comp;                          // [rows]: a member row of the row's component
    unsigned char *done;                // [rows]: by component id
    int *edge_u, *edge_v;               // [rows]: slot c is the edge component c hooked with
    float *edge_val;
    int *state;                         // components, merged, rounds, the hooks of the running round
    unsigned long long *part;           // [rows, parts]: workspace from here on
    unsigned long long *rbest;          // [rows]
    unsigned long long *cedge;          // [rows]: by component id
    unsigned *cbest;                    // [rows]: by component id
    int *parent;                        // [rows]: by component id
    long long rows, tiles, per;         // part s covers tiles [s * per, min(tiles, (s + 1) * per))
    float floor;
    int parts;
    const float *core;                  // [rows]: LINKAGE_REACH
};

#define LINKAGE_NO_EDGE 0xFFFFFFFFFFFFFFFFull
#define LINKAGE_PLAIN 0
#define LINKAGE_REACH 1

template <int KS, bool PF, int MODE, bool PFC = PF>
__global__ __launch_bounds__(256) void linkage_scan_kernel(LinkageArgs p) {
    constexpr int NF = 2 * KS, DIM = 64 * KS;
    constexpr bool REACH = MODE == LINKAGE_REACH;
    constexpr int NC = REACH ? 16 : 1;                                   // core values beside a tile's weights
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const long long q0 = ((long long)blockIdx.x * 4 + wave) * SEARCH_QW;
    if (q0 >= p.rows || p.state[1] == 0) return;                         // whole wavefronts leave: nothing below synchronises a block
    const bool live = q0 + l31 < p.rows;                                 // this lane's row exists
    const long long last_row = p.rows - 1;
    const long long qrow = min(q0 + l31, last_row);
    const int mine = p.comp[qrow];
    const bool active = live && p.done[mine] == 0;

    float bestv = __uint_as_float(0x7fc00000u);                          // NaN: !(v <= bestv) holds for every v
    int bestg = -1;

    if (__any(active)) {
        const long long t_begin = (long long)blockIdx.y * p.per, t_end = min(p.tiles, t_begin + p.per);
        v4i qf[NF];
        {
            const int8_t *src = p.x + (size_t)qrow * DIM + 16 * half;
#pragma unroll
            for (int f = 0; f < NF; ++f) qf[f] = *reinterpret_cast<const v4i *>(src + 32 * f);
        }
        const float qw = p.weight ? p.weight[qrow] : 1.0f;
        const float flr = p.floor;
        float cq = 0.0f;                                                 // REACH: this row's core similarity, the bound of its m
        unsigned act = 0u;                                               // REACH: the active rows of the wavefront, a bit per row
        if constexpr (REACH) {
            cq = p.core[qrow] + 0.0f;
            const unsigned long long b = __ballot(active);
            act = (unsigned)b | (unsigned)(b >> 32);
        }
        auto load_core = [&](long long g0, float (&c)[NC]) {
#pragma unroll
            for (int r = 0; r < NC; ++r) c[r] = p.core[min(g0 + scan_tile_row(r, half), last_row)];
        };
        auto load_tile = [&](long long g0, v4i (&a)[NF], float (&w)[16]) {
            const int8_t *src = p.x + (size_t)min(g0 + l31, last_row) * DIM + 16 * half;
#pragma unroll
            for (int f = 0; f < NF; ++f) a[f] = *reinterpret_cast<const v4i *>(src + 32 * f);
#pragma unroll
            for (int r = 0; r < 16; ++r) w[r] = p.weight ? p.weight[min(g0 + scan_tile_row(r, half), last_row)] : 1.0f;
        };

        v4i a[NF];
        float w[16];
        float c[NC];
        if constexpr (PF) load_tile(t_begin * SEARCH_TILE, a, w);
        if constexpr (REACH && PFC) load_core(t_begin * SEARCH_TILE, c);
        for (long long t = t_begin; t < t_end; ++t) {
            const long long g0 = t * SEARCH_TILE;
            v4i an[PF ? NF : 1];
            float wn[PF ? 16 : 1];
            float cn[REACH && PFC ? 16 : 1];
            if constexpr (PF) load_tile(min(t + 1, t_end - 1) * SEARCH_TILE, an, wn);         // no next tile: this one again, from the cache
            else load_tile(g0, a, w);
            if constexpr (REACH && PFC) load_core(min(t + 1, t_end - 1) * SEARCH_TILE, cn);
            else if constexpr (REACH) load_core(g0, c);
            v16i acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0;
#pragma unroll
            for (int f = 0; f < NF; ++f) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[f], qf[f], acc, 0, 0, 0);

            const int nrow = active ? scan_nrow(p.rows, g0) : 0; // rows of this tile inside the array
            // tile row `row` is row g = g0 + row of the array: g > b exactly when row > b - g0
            const int diag = scan_diag(q0 + l31 - g0);
            float v[16];
            unsigned mask = 0u;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = scan_tile_row(r, half);
                const bool up = row > diag;                              // the larger row's weight first
                v[r] = scan_pair_value(acc[r], w[r], qw, up);
                if constexpr (REACH) v[r] += 0.0f;                       // -0.0 -> +0.0 before any minimum
                if (row < nrow && v[r] >= flr && !(v[r] <= bestv)) mask |= 1u << r;
            }
            if (__any(mask != 0u)) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {                           // ascending g; row < nrow: inside the array
                    const int g = scan_tile_row(r, half, (int)g0);
                    if constexpr (REACH) {
                        if ((mask & (1u << r)) && !(v[r] <= bestv)) {
                            const float m = fminf(fminf(v[r], cq), c[r]) + 0.0f;
                            if (m >= flr && !(m <= bestv) && p.comp[g] != mine) {
                                bestv = m;
                                bestg = g;
                            }
                        }
                    } else if ((mask & (1u << r)) && !(v[r] <= bestv) && p.comp[g] != mine) {
                        bestv = v[r];
                        bestg = g;
                    }
                }
            }
            if constexpr (REACH) {                                       // the saturation exit: behind the reads of the accumulators
                const unsigned long long b = __ballot(bestg >= 0 && bestv == cq);
                if ((((unsigned)b | (unsigned)(b >> 32)) & act) == act) break;
            }
            if constexpr (PF) {
#pragma unroll
                for (int f = 0; f < NF; ++f) a[f] = an[f];
#pragma unroll
                for (int r = 0; r < 16; ++r) w[r] = wn[r];
            }
            if constexpr (REACH && PFC) {
#pragma unroll
                for (int r = 0; r < 16; ++r) c[r] = cn[r];
            }
        }
    }

    unsigned long long key = bestg >= 0 ? topk_key(bestv, bestg) : 0ull;
    const unsigned long long other = __shfl_xor(key, 32);                // the two lanes of a row; every lane of the wavefront is here
    key = other > key ? other : key;
    if (half == 0 && live) {
        p.part[(size_t)(q0 + l31) * p.parts + blockIdx.y] = key;
        if (blockIdx.y == 0) {                                           // every row has exactly one wavefront in part 0
            p.cbest[q0 + l31] = 0u;
            p.cedge[q0 + l31] = LINKAGE_NO_EDGE;
            if (q0 + l31 == 0) p.state[3] = 0;
        }
    }
}

__global__ __launch_bounds__(256) void linkage_fold_kernel(LinkageArgs p) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= p.rows || p.state[1] == 0) return;
    const unsigned long long *src = p.part + (size_t)q * p.parts;
    unsigned long long key = src[0];
    for (int s = 1; s < p.parts; ++s) key = src[s] > key ? src[s] : key;
    p.rbest[q] = key;
    if (key != 0ull) {
        unsigned *dst = p.cbest + p.comp[q];
        const unsigned u = (unsigned)(key >> 32);
        if (__hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < u) atomicMax(dst, u);
    }
}

__global__ __launch_bounds__(256) void linkage_pick_kernel(LinkageArgs p) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= p.rows || p.state[1] == 0) return;
    const unsigned long long key = p.rbest[q];
    if (key == 0ull) return;
    const int c = p.comp[q];
    if ((unsigned)(key >> 32) != p.cbest[c]) return;
    const unsigned g = 0xFFFFFFFFu - (unsigned)key, b = (unsigned)q;
    atomicMin(p.cedge + c, ((unsigned long long)min(b, g) << 32) | max(b, g));
}

__global__ __launch_bounds__(256) void linkage_hook_kernel(LinkageArgs p) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p.state[1] == 0) return;                                         // uniform: whole blocks leave
    bool hooked = false;
    if (c < p.rows && p.comp[c] == (int)c) {
        int root = (int)c;
        if (p.done[c] == 0) {
            const unsigned long long e = p.cedge[c];
            if (e == LINKAGE_NO_EDGE) {
                p.done[c] = 1;
            } else {
                const int i = (int)(e >> 32), j = (int)(unsigned)e;
                const int ci = p.comp[i];
                const int d = ci == (int)c ? p.comp[j] : ci;             // the component of the far end
                if (!(p.cedge[d] == e && (int)c < d)) {                  // two components that chose each other: the smaller id stays
                    root = d;
                    hooked = true;
                    p.edge_u[c] = i;
                    p.edge_v[c] = j;
                    p.edge_val[c] = topk_ordered_value(p.cbest[c]);
                }
            }
        }
        p.parent[c] = root;
    }
    const unsigned long long b = __ballot(hooked);
    if ((threadIdx.x & 63) == 0 && b != 0ull) atomicAdd(p.state + 3, __popcll(b));
}

__global__ __launch_bounds__(256) void linkage_jump_kernel(LinkageArgs p) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= p.rows || p.state[1] == 0) return;
    const int *__restrict__ parent = p.parent;
    int c = p.comp[q];
    for (int n = parent[c]; n != c; n = parent[c]) c = n;                // roots point at themselves
    p.comp[q] = c;
}

__global__ void linkage_finish_kernel(int *state) {
    if (state[1] == 0) return;
    const int hooks = state[3];
    state[0] -= hooks;
    state[1] = hooks;
    state[2] += hooks != 0;
}

__global__ __launch_bounds__(256) void linkage_init_kernel(LinkageArgs p) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= p.rows) return;
    p.comp[q] = (int)q;
    p.done[q] = 0;
    p.edge_u[q] = -1;
    p.edge_v[q] = -1;
    p.edge_val[q] = 0.0f;
    if (q == 0) {
        p.state[0] = (int)p.rows;
        p.state[1] = 1;
        p.state[2] = 0;
        p.state[3] = 0;
    }
}
