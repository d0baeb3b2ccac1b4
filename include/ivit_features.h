/*
 * ivit_features.h — the reference's forward_features (models/vit_quant.py:254-276, models/swin_quant.py:540-556) on the native
 * runners: the pre-head representation of every image and its scale, for retrieval, a linear probe, a second head on the same
 * backbone, or a comparison with the reference site by site.  Third public header of libivit_hip.so.
 *
 * Why a third header: ivit.h is frozen at IVIT_VERSION 111 and ivit_eval.h at IVIT_EVAL_VERSION 1 (their prototypes and versions
 * are pinned by the binding's tests), so these entries are declared here, under a version of their own.  This header includes
 * ivit.h and uses its handles (ivit_handle, ivit_vit, ivit_swin, ivit_graph), its status codes and every one of its conventions:
 * device pointers unless a name ends in _host, dense row-major tensors, asynchronous on the handle's HIP stream, nothing
 * allocated, nothing synchronised, hipGraph-capturable, IVIT_OK or an error code; a pointer named in an "Alignment:" line is
 * refused with IVIT_ERR_INVALID unless aligned, before anything is launched, and ivit_last_error names the argument.
 *
 * What it replaces:
 *   vit_quant.py:271-273    x = self.norm(x) ; x = x[:, 0] ; x, s = self.qact2(x)      the class-token row after norm -> qact2
 *   swin_quant.py:553-555   x = self.avgpool(x) ; x, s = self.qact3(x)                 the pooled row after qact3
 *   quant_modules.py:197-206  QuantAct returns integer * scale as an fp32 tensor       IVIT_FEATURES_DEQUANT
 * pre_logits (vit_quant.py:274) is the identity in every factory and is not part of this.
 */
#ifndef IVIT_FEATURES_H
#define IVIT_FEATURES_H

#include "ivit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: ivit_features_f32, ivit_vit_features, ivit_swin_features, ivit_vit_features_graph_create, ivit_swin_features_graph_create. */
#define IVIT_FEATURES_VERSION 1

/* mode of the fp32 form */
#define IVIT_FEATURES_DEQUANT 0
#define IVIT_FEATURES_UNIT 1

/* ---- f1  the fp32 form of int8 features: feat8 int8 [batch, dim], scale a HOST value -> out float [batch, dim].  Bit-exact:
 *   IVIT_FEATURES_DEQUANT  out[b, c] = fl32(fl32(feat8[b, c]) * scale): one conversion and one fp32 multiply, nothing contracted —
 *                          the bits of the fp32 tensor QuantAct returns in the reference.
 *   IVIT_FEATURES_UNIT     unit Euclidean length; the scale cancels and is not read.  ss[b] = sum_c q^2 as an exact integer,
 *                          out[b, c] = fl32((double)q / sqrt((double)ss[b])) with the fp64 square root and division correctly
 *                          rounded, so the only other rounding is the final fp64 -> fp32.  A row of zeros gives zeros, never NaN.
 * dim a multiple of 16 and at most 65536 (ss fits 31 bits): IVIT_ERR_UNSUPPORTED otherwise.  batch >= 0 (0 launches nothing),
 * dim >= 1, mode one of the two, scale finite and positive (checked in both modes): IVIT_ERR_INVALID otherwise.  feat8 is not
 * written.  One launch, one wavefront per row (csrc/ivit_features.h).                                                              */
/* Alignment: feat8 and out 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
int ivit_features_f32(ivit_handle h, const int8_t *feat8, int batch, int dim, float scale, int mode, float *out);

/* forward_features as one call: the runner of ivit_vit_forward / ivit_swin_forward with the same images, batch, nslices and
 * workspace (ivit_*_workspace_bytes and ivit_*_workspace_init are unchanged: a workspace made for forward serves features), which
 * leaves in
 *   feat8   int8 [batch, num_features] the integers the head reads: for a ViT (num_features = embed_dim) those of x[:, 0] after
 *           norm -> qact2, for a Swin (num_features = embed_dim << (num_layers - 1)) those after avgpool -> qact3.  Required.
 *           Each slice's final LayerNorm / pool writes its own rows there directly; the same integers for every nslices.
 *   logits  int32 [batch, num_classes], may be NULL.  Non-NULL: the head runs too and logits receives what ivit_*_forward writes,
 *           the same integers.  NULL: the head GEMM is not launched.
 *   feat32  float [batch, num_features], may be NULL.  Non-NULL: ivit_features_f32(feat8, batch, num_features, scale, mode,
 *           feat32) as ONE launch on the handle's stream behind the slices' join.  scale is a HOST value — the caller's copy of
 *           the scale of qact2 (ViT) / qact3 (Swin) — used only then, and then it must be finite and positive in both modes.
 * Every argument is checked before anything is launched: feat8 NULL, mode outside {0, 1}, a feat32 with a bad scale or a
 * misaligned pointer are IVIT_ERR_INVALID.  num_features is a multiple of 16 in every configuration, so with an aligned feat8
 * every slice's rows are aligned too.  The *_graph_create forms capture the same sequence (replay: ivit_graph_launch).             */
/* Alignment: feat8 and feat32 16-byte aligned, workspace 256-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
int ivit_vit_features(ivit_vit m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits,
                      int8_t *feat8, float scale, int mode, float *feat32);
int ivit_swin_features(ivit_swin m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits,
                       int8_t *feat8, float scale, int mode, float *feat32);
int ivit_vit_features_graph_create(ivit_vit m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes,
                                   int32_t *logits, int8_t *feat8, float scale, int mode, float *feat32, ivit_graph *out);
int ivit_swin_features_graph_create(ivit_swin m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes,
                                    int32_t *logits, int8_t *feat8, float scale, int mode, float *feat32, ivit_graph *out);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_FEATURES_H */
