/*
 * ivit_hidden.h — hidden states: the outputs of chosen blocks of a ViT / DeiT and of chosen stages of a Swin, from the native
 * runner.  What a backbone's user takes from it: get_intermediate_layers / forward_intermediates of a ViT, the four-stage feature
 * pyramid of a Swin.  Sixth public header of libivit_hip.so.
 *
 * The site.  Every block of both models closes with a 16-bit QuantAct over its second residual sum, qact4: it covers EVERY token
 * and has one per-tensor scale.  Its integers are the residual stream the runner carries from block to block; its scale is a host
 * float the model was created with (the input scale of whatever reads the stream next).  So a block's output is handed out in the
 * reference's own integers, and its fp32 form is the reference's tensor bit for bit.  (The sites the older headers left out stay
 * out: a ViT's patch rows behind the FINAL norm carry no scale, and nothing inside a Swin stage is tapped.)
 *
 * Why a sixth header: ivit.h is frozen at IVIT_VERSION 111, ivit_eval.h at IVIT_EVAL_VERSION 1, ivit_features.h at
 * IVIT_FEATURES_VERSION 1, ivit_attnmap.h at IVIT_ATTNMAP_VERSION 1 and ivit_classmap.h at IVIT_CLASSMAP_VERSION 1 (their
 * prototypes and versions are pinned by the binding's tests), so these entries are declared here, under a version of their own.
 * This header includes ivit.h and uses its handles (ivit_handle, ivit_vit, ivit_swin, ivit_graph), its status codes and every one
 * of its conventions: device pointers unless a name ends in _host, dense row-major tensors, asynchronous on the handle's HIP
 * stream, nothing allocated, nothing synchronised, hipGraph-capturable, IVIT_OK or an error code; a pointer named in an
 * "Alignment:" line is refused with IVIT_ERR_INVALID unless aligned, and a pair named in an "Overlap:" line unless disjoint
 * (ivit_last_error then contains "overlap" and both names), before anything is launched.
 *
 * What it stands for:
 *   vit_quant.py:130-143      Block.forward: ... x = x + drop_path(mlp(...)); x, s = self.qact4(x, s, x_2, s_2)    :141-143 the site
 *   swin_quant.py             SwinTransformerBlock.forward: the same closing qact4 (16 bit) over the second residual sum
 *   swin_quant.py             BasicLayer.forward: the blocks of a stage, THEN downsample (PatchMerging): a stage's output is the
 *                             output of its last block, in front of the merge
 *   quant_modules.py:204-206  QuantAct.forward returns x = q * s: the integers times the per-tensor scale, one fp32 multiply
 *
 * The definition (ivit_amd/predict.py: hidden_reference is the numpy statement):
 *   hid32 = fl32(fl32(q) * scale)      q an int16 of the stream (exactly convertible), scale the site's fp32 scale: ONE multiply
 *   layout IVIT_HIDDEN_TOKENS          [batch, T - t0, C]: token-major, as the stream lies in memory
 *   layout IVIT_HIDDEN_GRID            [batch, C, T - t0]: channel-major; the caller views the last axis as gh x gw (NCHW)
 *
 * Deliberately not here: patch rows behind a ViT's final norm; taps inside a Swin stage; the per-output norms detection frameworks
 * add; attention rollout; resizing; half-precision output forms; a CPU twin.
 */
#ifndef IVIT_HIDDEN_H
#define IVIT_HIDDEN_H

#include "ivit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: ivit_hidden_f32, ivit_vit_hidden_scale, ivit_swin_hidden_scale, ivit_vit_hidden_states, ivit_vit_hidden_states_graph_create,
 *    ivit_swin_hidden_states, ivit_swin_hidden_states_graph_create. */
#define IVIT_HIDDEN_VERSION 1

/* layout of the fp32 form */
#define IVIT_HIDDEN_TOKENS 0 /* [batch, T - t0, C] */
#define IVIT_HIDDEN_GRID 1   /* [batch, C, T - t0] */

/* ---- d1  the stateless operator: x16 int16 [batch, T, C] (a residual stream), scale a host float passed by value -> out float:
 * rows t0 .. T - 1 of every image as fl32(fl32(q) * scale), every fp32 bit the reference's (quant_modules.py:204-206); layout
 * IVIT_HIDDEN_TOKENS writes out [batch, T - t0, C], IVIT_HIDDEN_GRID out [batch, C, T - t0].  t0 = 1 drops a ViT's class row.
 * x16 is not written.  batch, T, C >= 1, 0 <= t0 < T, scale finite and positive, layout one of the two, x16 / out non-null:
 * IVIT_ERR_INVALID otherwise.  C a multiple of 8 (16-byte loads): IVIT_ERR_UNSUPPORTED otherwise.  One launch
 * (csrc/ivit_hidden.h): TOKENS a stream, GRID a transposition through LDS.                                                          */
/* Alignment: x16 and out 16-byte aligned: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: out may not overlap x16: IVIT_ERR_INVALID, nothing launched. */
int ivit_hidden_f32(ivit_handle h, const int16_t *x16, float scale, int batch, int T, int C, int t0, int layout, float *out);

/* ---- d2  the scale of a site, from what the model was created with: of blocks.{block}.qact4 of a ViT (the next block's s_ln1;
 * s_ln behind the last block), of the output of stage `stage` of a Swin (the next block's s_in inside a stage, the merge's s_in
 * behind one, s_norm_in behind the last).  Host queries: nothing is launched.  block outside [0, depth) / stage outside
 * [0, num_layers) or a null scale_host: IVIT_ERR_INVALID.                                                                           */
/* Alignment: none (scale_host is a host pointer). */
/* Overlap: none. */
int ivit_vit_hidden_scale(ivit_vit m, int block, float *scale_host);
/* Alignment: none (scale_host is a host pointer). */
/* Overlap: none. */
int ivit_swin_hidden_scale(ivit_swin m, int stage, float *scale_host);

/* ---- d3  the runner of ivit_vit_forward with the outputs of chosen blocks handed out: the same images, batch, nslices and
 * workspace (ivit_vit_workspace_bytes is unchanged: a workspace made for forward serves here), and
 *   blocks_host  nblocks block indices, strictly ascending in [0, depth) (a host array, read during the call)
 *   hid16        int16 [nblocks, batch, T, D], required: plane j holds the integers of blocks.{blocks_host[j]}.qact4, class row
 *                included.  The LAST launch of a tapped block writes its slice's rows here instead of into the workspace: no copy
 *                launch, no extra traffic; the next block reads them from here.  The same integers for every nslices.
 *   layout, hid32  hid32 NULL, or float: [nblocks, batch, T, D] for IVIT_HIDDEN_TOKENS, [nblocks, batch, D, T - 1] for
 *                IVIT_HIDDEN_GRID (patch rows only: the class token has no place on the grid).  One d1 launch per plane on the
 *                handle's stream behind the slices' join, with the scale of d2.
 *   logits       int32 [batch, num_classes]; non-NULL: what ivit_vit_forward writes, the same integers.  NULL: every slice
 *                returns behind its last tapped block.
 * A forward that taps block depth - 1 runs that block on all rows (the class-token tail of ivit_vit_cls_tail computes B rows only);
 * everything behind the attention is row-local, so the logits are the same integers.  ivit_vit_cls_tail keeps reporting what
 * forward does.  Every argument is checked before anything is launched: a NULL hid16, an empty or non-ascending list, an index out
 * of range, a layout outside {0, 1} with hid32 set are IVIT_ERR_INVALID; so is a model whose T * D is not a multiple of 8.
 * The *_graph_create form captures the same sequence (replay: ivit_graph_launch); a replay reads images as they are then.           */
/* Alignment: workspace 256-byte aligned, hid16 and hid32 16-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: images, workspace, logits, hid16 and hid32 must be pairwise disjoint: IVIT_ERR_INVALID, nothing launched. */
int ivit_vit_hidden_states(ivit_vit m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits,
                           const int *blocks_host, int nblocks, int16_t *hid16, int layout, float *hid32);
/* Alignment: as ivit_vit_hidden_states. */
/* Overlap: as ivit_vit_hidden_states. */
int ivit_vit_hidden_states_graph_create(ivit_vit m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes,
                                        int32_t *logits, const int *blocks_host, int nblocks, int16_t *hid16, int layout,
                                        float *hid32, ivit_graph *out);

/* ---- d4  the same of ivit_swin_forward, by stage:
 *   stages_host  nstages stage indices, strictly ascending in [0, num_layers)
 *   hid16        int16, required: plane j is the output of the last block of stage stages_host[j], in front of PatchMerging
 *                (BasicLayer.forward), [batch, L_s, C_s] with L_s = (grid >> s)^2 row-major over that stage's grid and
 *                C_s = embed_dim << s.  The planes are packed one after another: plane j starts at the sum of the earlier planes'
 *                batch * L * C elements.  Behind a tapped stage the merge's reduction writes the next stage's stream into the
 *                workspace, never into the caller's plane.
 *   layout, hid32  hid32 NULL, or float packed the same way: a plane is [batch, L_s, C_s] for IVIT_HIDDEN_TOKENS, [batch, C_s, L_s]
 *                for IVIT_HIDDEN_GRID.  One d1 launch per plane behind the slices' join.
 *   logits       as in d3; NULL: every slice returns behind its last tapped stage.
 * The checks and the *_graph_create form as in d3.                                                                                  */
/* Alignment: workspace 256-byte aligned, hid16 and hid32 16-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: images, workspace, logits, hid16 and hid32 must be pairwise disjoint: IVIT_ERR_INVALID, nothing launched. */
int ivit_swin_hidden_states(ivit_swin m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits,
                            const int *stages_host, int nstages, int16_t *hid16, int layout, float *hid32);
/* Alignment: as ivit_swin_hidden_states. */
/* Overlap: as ivit_swin_hidden_states. */
int ivit_swin_hidden_states_graph_create(ivit_swin m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes,
                                         int32_t *logits, const int *stages_host, int nstages, int16_t *hid16, int layout,
                                         float *hid32, ivit_graph *out);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_HIDDEN_H */
