// ivit_probe.h — linear probe (include/ivit_probe.h): the three exact integer statistics of a batch of labelled int8 features, ADDED
// into the caller's int64 buffers.  Two kernels, two launches per call, no workgroup waits for another, no workspace.
//
//   gram[i, j] += sum_r x[r, i] x[r, j]     class_sum[labels[r], :] += x[r, :]     count[labels[r]] += 1
//   over the rows with 0 <= labels[r] < num_classes (the comparison on all 64 bits of the label); every other row counts for nothing.
//
// probe_gram_kernel  The product contracts over ROWS: an operand of v_mfma_i32_32x32x32_i8 wants, per lane, 16 consecutive rows of ONE
//   feature column, while memory is contiguous along the features.  Grid (pairs of column blocks BI <= BJ) x (parts of the rows); a
//   column block is 128 features, a workgroup four wavefronts.  The workgroup walks its part 64 rows at a time.  Thread t loads
//   16 bytes (features 16 cg .. + 15 of its side: cg < 8 block BI, cg >= 8 block BJ) of each of the rows 4 rg .. 4 rg + 3 (cg = t % 16,
//   rg = t / 16), a row whose label is out of range or that lies beyond the part as zeros; transposes the four 4 x 4 byte blocks in
//   registers (probe_transpose4: eight v_perm_b32) and stores sixteen dwords — four rows of one column each — into the [column][row]
//   image in LDS.  Column c of the image begins at 80 c + 16 (c / 16): 64 row bytes and a pad that keeps every 16-byte read aligned
//   and spreads the sixteen column groups of a wavefront's stores over all banks.  The loads of the NEXT 64 rows are issued before
//   the MFMAs of these.  Wavefront w then reads, per 32 rows, ONE A operand (columns 32 w .. + 31 of block BI) and four B operands
//   (the four column tiles of block BJ) with 16-byte LDS reads — A and B come out of the same image, the operand lane map is the one
//   ivit_search.h relies on — and keeps a 32 x 128 strip of the 128 x 128 block in 64 int32 accumulators.
//   int32: a product is at most 2^14, so an accumulator holds 131 071 rows; it is added into the int64 matrix and cleared every
//   PROBE_FLUSH_ROWS = 65 536 rows (and at the end of the part).  Sums of different workgroups meet in the plain C++ atomicAdd on
//   unsigned long long (a vector global atomic; two's complement: the sign needs nothing).  A block pair off the diagonal adds its
//   block and the mirror image; a diagonal pair computes all 16 tiles of its block and adds them once.  Columns >= dim (dim = 192:
//   half of block 1) are loaded as zeros and never added.
//
// probe_class_kernel<LDS>  class_sum and count.  One thread per (row, 16 features).  LDS = true, where num_classes * (dim + 1) int32
//   fit 64 KB: the workgroup adds into its own zeroed LDS copy (ds_add_u32) and adds the copy's non-zero words into the int64 arrays
//   once per PROBE_FLUSH_ROWS rows — few classes are the case where every row of the batch meets the same few hundred addresses, and
//   64-bit global atomics to ONE address serialise.  LDS = false (many classes): straight 64-bit global atomicAdd per feature; the
//   rows spread over num_classes * dim addresses.
// Integers throughout: the result depends neither on the grid nor on any order.  Plain vector stores and atomics only, no scratch.
#pragma once
#include "../../include/ivit_probe.h"
#include "ivit_device.h"

#define PROBE_MIN_DIM 64
#define PROBE_MAX_DIM 1024
#define PROBE_MAX_CLASSES 65536
#define PROBE_BLK 128                              // features of a column block
#define PROBE_CHUNK 64                             // rows of one LDS image: two k-steps of the MFMA
#define PROBE_COL_BYTES 80                         // image bytes of a column: 64 rows + 16
#define PROBE_IMAGE_BYTES (2 * PROBE_BLK * PROBE_COL_BYTES + (2 * PROBE_BLK / 16) * 16)
#define PROBE_FLUSH_ROWS 65536                     // rows an int32 accumulator takes before it is added into the int64 total (< 131 072)
#define PROBE_CLASS_LDS_BYTES 65536

__host__ __device__ __forceinline__ int probe_image_offset(int col, int row) { return col * PROBE_COL_BYTES + (col >> 4) * 16 + row; }

struct ProbeArgs {
    const int8_t *feat8;            // [rows, dim]
    const long long *labels;        // [rows]
    unsigned long long *gram;       // [dim, dim]
    unsigned long long *class_sum;  // [num_classes, dim]
    unsigned long long *count;      // [num_classes]
    long long rows, per;            // part s covers rows [s * per, min(rows, (s + 1) * per)); per is a multiple of PROBE_CHUNK
    int dim, num_classes, nblk;     // nblk: column blocks, ceil(dim / 128)
};

__device__ __forceinline__ bool probe_label_ok(long long label, int num_classes) {
    return (unsigned long long)label < (unsigned long long)num_classes;                      // all 64 bits: 2^32 + 3 is no class
}

// a0 .. a3: four consecutive rows' dwords (four features each) -> o[c]: the four rows' bytes of feature c, row 0 lowest
__device__ __forceinline__ void probe_transpose4(unsigned a0, unsigned a1, unsigned a2, unsigned a3, unsigned (&o)[4]) {
    const unsigned t0 = __builtin_amdgcn_perm(a1, a0, 0x05010400u);      // a0.b0 a1.b0 a0.b1 a1.b1
    const unsigned t1 = __builtin_amdgcn_perm(a1, a0, 0x07030602u);      // a0.b2 a1.b2 a0.b3 a1.b3
    const unsigned u0 = __builtin_amdgcn_perm(a3, a2, 0x05010400u);
    const unsigned u1 = __builtin_amdgcn_perm(a3, a2, 0x07030602u);
    o[0] = __builtin_amdgcn_perm(u0, t0, 0x05040100u);                   // a0.b0 a1.b0 a2.b0 a3.b0
    o[1] = __builtin_amdgcn_perm(u0, t0, 0x07060302u);
    o[2] = __builtin_amdgcn_perm(u1, t1, 0x05040100u);
    o[3] = __builtin_amdgcn_perm(u1, t1, 0x07060302u);
}

__global__ __launch_bounds__(256) void probe_gram_kernel(ProbeArgs p) {
    __shared__ __attribute__((aligned(16))) char image[PROBE_IMAGE_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const long long r_begin = (long long)blockIdx.y * p.per, r_end = min(p.rows, r_begin + p.per);
    if (r_begin >= r_end) return;                                        // the whole workgroup leaves
    int bi = 0, bj = (int)blockIdx.x;                                    // pair index -> (bi, bj), bi <= bj, row by row of the upper triangle
    while (bj >= p.nblk - bi) { bj -= p.nblk - bi; ++bi; }
    bj += bi;

    const int cg = tid & 15, rg = tid >> 4;                              // this thread's 16 features and 4 rows of every chunk
    const int col0 = (cg < 8 ? bi * PROBE_BLK : bj * PROBE_BLK - PROBE_BLK) + 16 * cg;        // its first feature
    const bool col_ok = col0 < p.dim;
    const int8_t *src = p.feat8 + col0;
    char *dst = image + probe_image_offset(16 * cg, 4 * rg);

    auto load_rows = [&](long long r0, v4i (&x)[4]) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long long r = r0 + 4 * rg + q;
            x[q] = v4i{0, 0, 0, 0};
            if (col_ok && r < r_end && probe_label_ok(p.labels[r], p.num_classes))
                x[q] = *reinterpret_cast<const v4i *>(src + (size_t)r * p.dim);
        }
    };
    auto store_image = [&](const v4i (&x)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned o[4];
            probe_transpose4((unsigned)x[0][j], (unsigned)x[1][j], (unsigned)x[2][j], (unsigned)x[3][j], o);
#pragma unroll
            for (int c = 0; c < 4; ++c) *reinterpret_cast<unsigned *>(dst + (4 * j + c) * PROBE_COL_BYTES) = o[c];
        }
    };
    const char *a_src = image + probe_image_offset(32 * wave + l31, 16 * half);
    const char *b_src = image + probe_image_offset(PROBE_BLK + l31, 16 * half);
    constexpr int TILE_BYTES = 32 * PROBE_COL_BYTES + 2 * 16;           // from one 32-column tile of the image to the next

    v16i acc[4];
    auto clear = [&]() {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0;
    };
    auto flush = [&]() {
        const bool mirror = bi != bj;
        const int i0 = bi * PROBE_BLK + 32 * wave + 4 * half;            // A's columns: the accumulators', i0 + (r & 3) + 8 (r >> 2)
        if (i0 >= p.dim) return;                                         // dim is a multiple of 64: a 32-column tile is wholly in or out
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int j = bj * PROBE_BLK + 32 * t + l31;                 // B's column: the lane's
            if (j >= p.dim) continue;
            unsigned long long *own = p.gram + (size_t)i0 * p.dim + j, *mir = p.gram + (size_t)j * p.dim + i0;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int di = (r & 3) + 8 * (r >> 2);
                const unsigned long long v = (unsigned long long)(long long)acc[t][r];
                atomicAdd(own + (size_t)di * p.dim, v);
                if (mirror) atomicAdd(mir + di, v);
            }
        }
    };

    clear();
    v4i x[4];
    load_rows(r_begin, x);
    long long held = 0;                                                  // rows in the accumulators
    for (long long r0 = r_begin; r0 < r_end; r0 += PROBE_CHUNK) {
        __syncthreads();                                                 // the last chunk's reads are done
        store_image(x);
        __syncthreads();
        if (r0 + PROBE_CHUNK < r_end) load_rows(r0 + PROBE_CHUNK, x);    // in flight during the MFMAs
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const v4i a = *reinterpret_cast<const v4i *>(a_src + 32 * ks);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const v4i b = *reinterpret_cast<const v4i *>(b_src + t * TILE_BYTES + 32 * ks);
                acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc[t], 0, 0, 0);
            }
        }
        held += PROBE_CHUNK;
        if (held >= PROBE_FLUSH_ROWS) { flush(); clear(); held = 0; }
    }
    if (held) flush();
}

template <bool LDS>
__global__ __launch_bounds__(256) void probe_class_kernel(ProbeArgs p) {
    extern __shared__ __attribute__((aligned(16))) char probe_sm[];
    int *priv = reinterpret_cast<int *>(probe_sm);                       // LDS: [num_classes, dim] sums, then [num_classes] counts
    const int pieces = p.dim >> 4, nsum = p.num_classes * p.dim, nall = nsum + p.num_classes;
    const long long r_begin = (long long)blockIdx.x * p.per, r_end = min(p.rows, r_begin + p.per);
    if (r_begin >= r_end) return;
    for (long long f0 = r_begin; f0 < r_end; f0 += PROBE_FLUSH_ROWS) {
        const long long f1 = min(r_end, f0 + PROBE_FLUSH_ROWS);
        if constexpr (LDS) {
            __syncthreads();
            for (int i = threadIdx.x; i < nall; i += 256) priv[i] = 0;
            __syncthreads();
        }
        const int n = (int)(f1 - f0) * pieces;                            // at most 65 536 * 64
        for (int w = threadIdx.x; w < n; w += 256) {
            const int piece = w % pieces;
            const long long r = f0 + w / pieces;
            const long long label = p.labels[r];
            if (!probe_label_ok(label, p.num_classes)) continue;
            const v4i v = *reinterpret_cast<const v4i *>(p.feat8 + (size_t)r * p.dim + 16 * piece);
            const size_t base = (size_t)label * p.dim + 16 * piece;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int q = (int)(signed char)((unsigned)v[j] >> (8 * b));
                    if constexpr (LDS) atomicAdd(priv + base + 4 * j + b, q);
                    else if (q) atomicAdd(p.class_sum + base + 4 * j + b, (unsigned long long)(long long)q);
                }
            if (piece == 0) {
                if constexpr (LDS) atomicAdd(priv + nsum + (int)label, 1);
                else atomicAdd(p.count + label, 1ull);
            }
        }
        if constexpr (LDS) {
            __syncthreads();
            for (int i = threadIdx.x; i < nall; i += 256) {
                const int s = priv[i];
                if (s) atomicAdd(i < nsum ? p.class_sum + i : p.count + (i - nsum), (unsigned long long)(long long)s);
            }
        }
    }
}
