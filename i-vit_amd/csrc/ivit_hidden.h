// ivit_hidden.h — the fp32 form of a block's or a stage's output (include/ivit_hidden.h, ivit_hidden_f32): the 16-bit residual stream
// x16 [batch, T, C] behind a block's closing QuantAct (qact4: vit_quant.py:141-143, SwinTransformerBlock.forward) times its per-tensor
// scale, the tensor QuantAct.forward returns in the reference (x = q * s, quant_modules.py:204-206):
//   out = fl32(fl32(q) * scale)      v_cvt_f32_i32 of an int16 (exact) and ONE multiply (the library is built with -ffp-contract=off)
// for the rows t0 .. T - 1 of every image (t0 = 1 drops a ViT's class row), N = T - t0 of them.
//
// hidden_f32_kernel<false>  TOKENS, out [batch, N, C]: a stream.  An image's rows t0 .. T - 1 are one contiguous run of N * C / 8
//   16-byte pieces (C is a multiple of 8 and x16 is 16-byte aligned): a thread loads a piece (global_load_dwordx4), converts its eight
//   integers and stores two float4.  Grid: x over the pieces of an image (grid-stride), y over the images (stride gridDim.y).  No LDS.
//
// hidden_f32_kernel<true>   GRID, out [batch, C, N]: a transposition through LDS, 64 tokens x 64 channels per workgroup pass, coalesced
//   along C on the way in (16-byte loads, a token's 128 bytes in one instruction) and along the tokens on the way out (a wavefront
//   stores 64 consecutive floats of one channel).  The tile is fp32 [64 tokens][HIDDEN_PITCH = 65]: cell (t, c) at dword t * 65 + c.
//   ds_write_b32 and ds_read_b32 bank on dword % 32 within each 32-lane half, and 65 % 32 = 1, so
//     write  lane l: half = l / 32, row tr = (l % 32) / 4, piece cg = 4 * half + l % 4; its j-th dword goes to (row0 + tr) * 65 + cg * 8 + j
//            (row0 = 32 * pass + 8 * wave): within a half tr = 0 .. 7 and (cg % 4) * 8 = 0, 8, 16, 24 -> bank (const + tr + 8 * (cg % 4)) % 32,
//            32 distinct banks for every j (the compiler pairs the eight stores into four ds_write2_b32: two such dwords per lane);
//     read   lane l reads token l of channel ch: l * 65 + ch -> bank (l + ch) % 32: 32 distinct banks within a half;
//   both are conflict-free by the rule.  Edge tiles in both directions: a lane whose token or piece lies outside the image neither loads
//   nor writes its cells, and a lane whose token or channel lies outside does not read or store; the two block barriers of a pass stand
//   outside every such branch (blockIdx, batch and the tile counts are uniform over the block).  Grid: x over the tiles of an image
//   (token tile fastest), y over the images (stride gridDim.y).  16 640 bytes of LDS.
// Plain vector stores only, no scratch.
#pragma once
#include "../../include/ivit_hidden.h"

#define HIDDEN_TILE 64       // tokens and channels of a GRID tile
#define HIDDEN_PITCH 65      // dwords between two token rows of the tile: odd

// the eight int16 of a 16-byte piece, scaled
__device__ __forceinline__ void hidden_piece(const v4i v, float scale, float (&o)[8]) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        o[2 * d] = (float)((v[d] << 16) >> 16) * scale;
        o[2 * d + 1] = (float)(v[d] >> 16) * scale;
    }
}

template <bool GRID>
__global__ __launch_bounds__(256) void hidden_f32_kernel(const int16_t *__restrict__ x16, float scale, int batch, int T, int C, int t0,
                                                         float *__restrict__ out) {
    const int N = T - t0;
    if constexpr (!GRID) {
        const long long per = (long long)N * (C >> 3);                       // 16-byte pieces of an image's rows t0 .. T - 1
        for (int b = blockIdx.y; b < batch; b += gridDim.y) {
            const v4i *src = reinterpret_cast<const v4i *>(x16 + ((size_t)b * T + t0) * C);
            float4 *dst = reinterpret_cast<float4 *>(out + (size_t)b * N * C);
            for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < per; p += (long long)gridDim.x * 256) {
                float o[8];
                hidden_piece(src[p], scale, o);
                dst[2 * p] = make_float4(o[0], o[1], o[2], o[3]);
                dst[2 * p + 1] = make_float4(o[4], o[5], o[6], o[7]);
            }
        }
    } else {
        __shared__ float tile[HIDDEN_TILE * HIDDEN_PITCH];
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int nt = (N + HIDDEN_TILE - 1) / HIDDEN_TILE;
        const int n0 = (int)(blockIdx.x % nt) * HIDDEN_TILE, c0 = (int)(blockIdx.x / nt) * HIDDEN_TILE;
        const int cg = 4 * (lane >> 5) + (lane & 3), tr = (lane & 31) >> 2;
        for (int b = blockIdx.y; b < batch; b += gridDim.y) {
            const int16_t *src = x16 + ((size_t)b * T + t0) * C;
            float *dst = out + (size_t)b * C * N;
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
                const int tok = pass * 32 + wave * 8 + tr, n = n0 + tok, c = c0 + cg * 8;
                if (n < N && c < C) {                                        // C is a multiple of 8: the whole piece lies inside
                    float o[8];
                    hidden_piece(*reinterpret_cast<const v4i *>(src + (size_t)n * C + c), scale, o);
#pragma unroll
                    for (int j = 0; j < 8; ++j) tile[tok * HIDDEN_PITCH + cg * 8 + j] = o[j];
                }
            }
            __syncthreads();
#pragma unroll 4
            for (int i = 0; i < HIDDEN_TILE / 4; ++i) {
                const int ch = wave * (HIDDEN_TILE / 4) + i, c = c0 + ch, n = n0 + lane;
                if (c < C && n < N) dst[(size_t)c * N + n] = tile[lane * HIDDEN_PITCH + ch];
            }
            __syncthreads();                                                 // the next image's pass writes the tile again
        }
    }
}
