/*
 * ivit_attnmap.h — what a ViT / DeiT looks at: the attention probabilities of the class token, the integers behind every
 * attention-map picture of such a model, from the native runner.  In the reference they are row 0 of IntSoftmax's output
 * (models/vit_quant.py:76, 16 bit, scale 2^-15) of the block one asks about; the fused attention kernels of this library keep
 * scores and probabilities in registers, so the row is produced by a small launch of its own, directly behind the block's qkv
 * launch.  Fourth public header of libivit_hip.so.
 *
 * Why a fourth header: ivit.h is frozen at IVIT_VERSION 111, ivit_eval.h at IVIT_EVAL_VERSION 1 and ivit_features.h at
 * IVIT_FEATURES_VERSION 1 (their prototypes and versions are pinned by the binding's tests), so these entries are declared here,
 * under a version of their own.  This header includes ivit.h and uses its handles (ivit_handle, ivit_vit, ivit_graph), its
 * ivit_dyadic, its status codes and every one of its conventions: device pointers unless a name ends in _host, dense row-major
 * tensors, asynchronous on the handle's HIP stream, nothing allocated, nothing synchronised, hipGraph-capturable, IVIT_OK or an
 * error code; a pointer named in an "Alignment:" line is refused with IVIT_ERR_INVALID unless aligned, and a pair named in an
 * "Overlap:" line unless disjoint (ivit_last_error then contains "overlap" and both names), before anything is launched.
 *
 * What it replaces:
 *   vit_quant.py:70-74        matmul_1(q, k^T), attn * self.scale, qact_attn1       the 8-bit scores, here of query 0 only
 *   vit_quant.py:76           attn = self.int_softmax(attn, ...)                    row 0 of [B, H, N, N]
 *   quant_modules.py:483-497  IntSoftmax.forward                                    the row's Shiftmax, bit for bit
 *
 * Deliberately not here: Swin (no class token: its windows attend among patches only, there is no one row to show); whole
 * T x T matrices (ivit_attn_qk_requant + ivit_shiftmax of ivit.h give them); attention rollout (a float product of those
 * matrices that the reference does not define); upsampling of a map to pixels.
 */
#ifndef IVIT_ATTNMAP_H
#define IVIT_ATTNMAP_H

#include "ivit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: ivit_attention_cls_probs, ivit_attention_map_f32, ivit_vit_attention, ivit_vit_attention_graph_create. */
#define IVIT_ATTNMAP_VERSION 1

/* mode of the fp32 map */
#define IVIT_ATTNMAP_HEADS 0
#define IVIT_ATTNMAP_MEAN 1

/* ---- m1  the class token's probabilities of one block: q, k int8 [B*H, T, dh] as every qkv entry of ivit.h writes them, dy_qk and
 * s_softmax the block's (the multiplier of qact_attn1 and its scale) -> p_cls uint16 [B*H, T], dense.  For every (image, head):
 *   acc[j] = q[bh, 0, :] . k[bh, j, :]   (int32),   sc8[j] = clamp8(rne((double(acc[j]) * m) * r))   — any multiplier —,
 *   p_cls[bh, :] = Shiftmax(sc8, s_softmax) at 16 bits, the sequence of ivit_shiftmax (row maximum, shift-exp, the row sum in torch's
 *   order, floor((2^31 - 1) / S), floor(e * F / 2^16)): the integers of row 0 of blocks.i.attn.int_softmax in the reference.
 * Replaces vit_quant.py:70-76 for the class-token row.  q and k are not written; of q only row 0 of every [T, dh] is read.
 * B, H, T, dh >= 1, all pointers non-null, s_softmax finite and positive: IVIT_ERR_INVALID otherwise.  dh a multiple of 16 and at
 * most 128, T at most 1024: IVIT_ERR_UNSUPPORTED otherwise.  One launch, one wavefront per (image, head) (csrc/ivit_attnmap.h).      */
/* Alignment: q and k 16-byte aligned (p_cls takes any uint16 address: 2-byte stores): IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: p_cls may not overlap q or k: IVIT_ERR_INVALID, nothing launched. */
int ivit_attention_cls_probs(ivit_handle h, const int8_t *q, const int8_t *k, ivit_dyadic dy_qk, float s_softmax,
                             uint16_t *p_cls, int B, int H, int T, int dh);

/* ---- m2  the fp32 map over the patches: p_cls uint16 [rows, H, T] -> float, columns j = 1 .. T - 1 only (column 0 is the class
 * token's attention to itself).  Bit-exact:
 *   IVIT_ATTNMAP_HEADS  out [rows, H, T - 1],  out[r, h, j - 1] = fl32(p[r, h, j]) * 2^-15, exact: the fp32 tensor IntSoftmax
 *                       returns in the reference (quant_modules.py:496-497: integer * 2^-15).
 *   IVIT_ATTNMAP_MEAN   out [rows, T - 1],  S = sum_h p[r, h, j] as an exact integer (at most H * 32768),
 *                       out[r, j - 1] = fl32(S) / fl32(H * 32768), the IEEE correctly rounded fp32 quotient: one rounding.
 * rows >= 0 and T = 1 launch nothing.  rows < 0, H < 1, T < 1, a null pointer or a mode outside {0, 1}: IVIT_ERR_INVALID.  H above
 * 511 (S must stay below 2^24) or T above 1024: IVIT_ERR_UNSUPPORTED.  p_cls is not written.  One launch.                          */
/* Alignment: p_cls 2-byte and out 4-byte aligned, their elements: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: out may not overlap p_cls: IVIT_ERR_INVALID, nothing launched. */
int ivit_attention_map_f32(ivit_handle h, const uint16_t *p_cls, int64_t rows, int H, int T, int mode, float *out);

/* ---- m3  the runner of ivit_vit_forward with the class-token rows of chosen blocks tapped: the same images, batch, nslices and
 * workspace (ivit_vit_workspace_bytes and ivit_vit_workspace_init are unchanged: a workspace made for forward serves here), and
 *   blocks_host  HOST array of nblocks block indices, 1 <= nblocks <= depth, strictly ascending, each in [0, depth):
 *                IVIT_ERR_INVALID otherwise.
 *   attn16   uint16 [nblocks, batch, H, T], required.  Plane t is row 0 of blocks.{blocks_host[t]}.attn.int_softmax
 *            (vit_quant.py:76) for every image and head: each slice issues ivit_attention_cls_probs for its images directly
 *            behind that block's qkv launch, whichever form the block's attention takes.  The same integers for every nslices.
 *   logits   int32 [batch, num_classes], may be NULL.  Non-NULL: the whole forward runs and logits receives what ivit_vit_forward
 *            writes, the same integers.  NULL: every slice ends behind the tap of the last tapped block; nothing after it is
 *            launched.
 *   map32    float, may be NULL.  Non-NULL: ivit_attention_map_f32(attn16, nblocks * batch, H, T, mode, map32) as ONE launch on
 *            the handle's stream behind the slices' join: [nblocks, batch, H, T - 1] or [nblocks, batch, T - 1] by mode.
 * Every argument is checked before anything is launched: attn16 NULL, a bad block list, a mode outside {0, 1} (judged with or
 * without map32) are IVIT_ERR_INVALID; a model whose head_dim or token count lies outside m1's limits is IVIT_ERR_UNSUPPORTED.
 * The *_graph_create form captures the same sequence (replay: ivit_graph_launch); blocks_host is read during the call only.      */
/* Alignment: workspace 256-byte aligned, attn16 2-byte, map32 4-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: images, workspace, logits, attn16 and map32 must be pairwise disjoint: IVIT_ERR_INVALID, nothing launched. */
int ivit_vit_attention(ivit_vit m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes,
                       int32_t *logits, const int *blocks_host, int nblocks, uint16_t *attn16, int mode, float *map32);
/* Alignment: as ivit_vit_attention. */
/* Overlap: as ivit_vit_attention. */
int ivit_vit_attention_graph_create(ivit_vit m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes,
                                    int32_t *logits, const int *blocks_host, int nblocks, uint16_t *attn16, int mode, float *map32,
                                    ivit_graph *out);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_ATTNMAP_H */
