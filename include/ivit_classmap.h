/*
 * ivit_classmap.h — what a Swin's decision rests on, token by token: class-activation maps in exact integers, and the dense
 * final-stage token features they are made of, from the native runner.  A Swin ends in
 *   norm -> qact2 -> global average pool -> qact3 -> linear head                                   (models/swin_quant.py:551-564)
 * and qact2 is applied to EVERY token, so the final-stage tokens tok8 [B, L, C] are int8 integers on one per-tensor scale (a
 * ViT's patch rows have no such scale: there the reference applies qact2 to the class row only).  The evidence of token t for class
 * c is the head's weight row against that token, head_w[c, :] . tok8[b, t, :], an int32 with no rounding anywhere.  Fifth public
 * header of libivit_hip.so.
 *
 * Why a fifth header: ivit.h is frozen at IVIT_VERSION 111, ivit_eval.h at IVIT_EVAL_VERSION 1, ivit_features.h at
 * IVIT_FEATURES_VERSION 1 and ivit_attnmap.h at IVIT_ATTNMAP_VERSION 1 (their prototypes and versions are pinned by the binding's
 * tests), so these entries are declared here, under a version of their own.  This header includes ivit.h and uses its handles
 * (ivit_handle, ivit_swin, ivit_graph), its status codes and every one of its conventions: device pointers unless a name ends in
 * _host, dense row-major tensors, asynchronous on the handle's HIP stream, nothing allocated, nothing synchronised,
 * hipGraph-capturable, IVIT_OK or an error code; a pointer named in an "Alignment:" line is refused with IVIT_ERR_INVALID unless
 * aligned, and a pair named in an "Overlap:" line unless disjoint (ivit_last_error then contains "overlap" and both names), before
 * anything is launched.
 *
 * What it stands for:
 *   swin_quant.py:551-552     x = self.norm(x, ...); x, act_scaling_factor = self.qact2(x, ...)     tok8 and its scale s_tok
 *   swin_quant.py:553-556     avgpool, qact3, flatten                                               what the head reads instead
 *   swin_quant.py:560-564     forward: x = self.head(x, act_scaling_factor)                         the weight rows, per class
 *   quant_modules.py:67-97    QuantLinear.forward: weight_integer, fc_scaling_factor, and
 *                             bias_scaling_factor = fc_scaling_factor * prev_act_scaling_factor     the unit of a map: class_scale
 *
 * The definition (ivit_amd/predict.py: class_map_reference is the numpy statement):
 *   cam32[b, j, t] = sum_c int(head_w[idx[b, j], c]) * int(tok8[b, t, c])       int32 [B, k, L], exact
 *   map32[b, j, t] = fl32(fl32(cam32[b, j, t]) * class_scale[idx[b, j]])        float32: the conversion is exact (|cam32| <=
 *                    128 * 127 * C < 2^24 for C <= 1024), then one fp32 multiply: the contract of ivit_logits_topk's v[b, c]
 *   class_scale[c] = fl32(s_tok * fc_scaling_factor[c]): quant_modules.py:96-97 with qact2's scale in place of qact3's, the unit
 *                    the head's output would have were the head applied to one token.  The caller builds it (SwinEngine.class_scale).
 * The maps explain the logits through one exact identity: sum_t cam32[b, j, t] == head_w[c] . sum_t tok8[b, t, :], and the pool's
 * requantisation of that token sum (swin_quant.py:553-555) is what the head reads — the sum of a map is logits - bias up to that
 * single requantisation.
 *
 * Deliberately not here: a ViT counterpart (its patch rows carry no scale); upsampling of a map to pixels; Grad-CAM or any other
 * gradient; maps of earlier stages (no head reads them).  A Swin still has no attention entry: it has no class token.
 */
#ifndef IVIT_CLASSMAP_H
#define IVIT_CLASSMAP_H

#include "ivit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: ivit_class_map, ivit_swin_class_map, ivit_swin_class_map_graph_create. */
#define IVIT_CLASSMAP_VERSION 1

/* mode of the runner: where the class indices come from */
#define IVIT_CLASSMAP_TOPK 0  /* idx (and val) are OUTPUTS: the k best classes of this forward */
#define IVIT_CLASSMAP_GIVEN 1 /* idx is an INPUT: the caller's classes, e.g. the labels        */

/* ---- c1  the maps of given classes: tok8 int8 [batch, L, C] (the tokens behind qact2), head_w int8 [num_classes, C] (the head's
 * weight_integer), idx int32 [batch, k] (read on the device: no host round trip) -> cam32 int32 [batch, k, L] and, with class_scale
 * float [num_classes], map32 float [batch, k, L], both as defined above, every integer and every fp32 bit.  An index outside
 * [0, num_classes) forms no address: its cam32 row is zeros and its map32 row NaN (0x7fc00000), the convention of ivit_logits_score
 * for a label out of range; duplicate indices in a row are allowed.  tok8, head_w, idx and class_scale are not written.
 * Stands for swin_quant.py:560-564 and quant_modules.py:67-97 applied to one token at a time, in front of the pool.
 * batch, L, k, num_classes >= 1, k <= 16, tok8 / head_w / idx / cam32 non-null, class_scale and map32 both NULL or both set:
 * IVIT_ERR_INVALID otherwise.  C a multiple of 16 and at most 1024 (cam32 must stay below 2^24): IVIT_ERR_UNSUPPORTED otherwise.
 * One launch, one wavefront per (image, class slot) (csrc/ivit_classmap.h).                                                          */
/* Alignment: tok8 and head_w 16-byte aligned, idx, class_scale, cam32 and map32 4-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: cam32 and map32 may overlap neither tok8, idx nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_class_map(ivit_handle h, const int8_t *tok8, const int8_t *head_w, const int32_t *idx, int batch, int L, int C,
                   int num_classes, int k, const float *class_scale, int32_t *cam32, float *map32);

/* ---- c2  the runner of ivit_swin_forward with the final-stage tokens handed out and the maps behind it: the same images, batch,
 * nslices and workspace (ivit_swin_workspace_bytes is unchanged: a workspace made for forward serves here), and
 *   tok8     int8 [batch, L, C], required: L the final stage's token count ((grid >> (num_layers - 1))^2, row-major over that grid),
 *            C = embed_dim << (num_layers - 1).  The final norm -> qact2 of every slice writes its rows here instead of into the
 *            workspace (swin_quant.py:551-552) and the pool reads them from here.  The same integers for every nslices.
 *   mode     IVIT_CLASSMAP_TOPK: logits, head_scale and idx are required, val may be NULL; behind the slices' join
 *            ivit_logits_topk(logits, head_scale, k, idx, val), 1 <= k <= min(16, num_classes), then c1 on those indices.
 *            IVIT_CLASSMAP_GIVEN: idx is read, 1 <= k <= 16; val must be NULL and head_scale is not read; logits may be NULL, and
 *            then every slice ends behind the final norm: neither the pool nor the head is launched.
 *   logits   int32 [batch, num_classes]; non-NULL: what ivit_swin_forward writes, the same integers.
 *   cam32    int32 [batch, k, L], required; map32 float [batch, k, L] and class_scale float [num_classes]: both or neither.
 * c1 is ONE launch on the handle's stream behind the slices' join, with the head's weights the model was created with.
 * Every argument is checked before anything is launched: a NULL tok8 / cam32 / idx, a mode outside {0, 1}, val in GIVEN mode,
 * NULL logits or head_scale in TOPK mode, k out of range, class_scale without map32 or the reverse are IVIT_ERR_INVALID; a model
 * whose C lies outside c1's limits is IVIT_ERR_UNSUPPORTED.  The *_graph_create form captures the same sequence (replay:
 * ivit_graph_launch); a replay reads images — and in GIVEN mode idx — as they are then.                                           */
/* Alignment: workspace 256-byte aligned, tok8 16-byte, idx, val, class_scale, cam32 and map32 4-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: images, workspace, logits, idx, val, tok8, cam32 and map32 must be pairwise disjoint (images against idx in GIVEN mode excepted: both are only read): IVIT_ERR_INVALID, nothing launched. */
int ivit_swin_class_map(ivit_swin m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes,
                        int32_t *logits, const float *head_scale, int mode, int k, int32_t *idx, float *val, int8_t *tok8,
                        const float *class_scale, int32_t *cam32, float *map32);
/* Alignment: as ivit_swin_class_map. */
/* Overlap: as ivit_swin_class_map. */
int ivit_swin_class_map_graph_create(ivit_swin m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes,
                                     int32_t *logits, const float *head_scale, int mode, int k, int32_t *idx, float *val,
                                     int8_t *tok8, const float *class_scale, int32_t *cam32, float *map32, ivit_graph *out);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_CLASSMAP_H */
