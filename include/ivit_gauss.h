/*
 * ivit_gauss.h — novelty scores: the squared Mahalanobis distance of int8 feature rows to the nearest class mean of a Gaussian model
 * with a shared covariance (linear discriminant analysis; with one class a plain novelty score), fused.  Seventeenth public header of
 * libivit_hip.so.
 *
 * Why an entry of its own: top-k, k-NN, range search, the probes and k-means answer WHICH class, neighbour or cluster; the question
 * behind a prediction at deployment is whether the image is like the training data at all.  The statistics of ivit_probe.h (Gram
 * matrix, class sums, counts) are exactly the sufficient statistics of this model, so the fit is a host computation
 * (ivit_amd/predict.py: gauss_fit_reference); what is left is scoring rows.  In a tensor library that is a [N, R] fp32 matrix of
 * whitened rows and a [N, C] matrix of class scores per batch; here neither is written.
 *
 * Why a seventeenth header: ivit.h is frozen at IVIT_VERSION 111 and the fifteen headers behind it at their versions (their
 * prototypes and versions are pinned by the binding's tests), so these entries are declared here, under a version of their own.  This
 * header includes ivit.h and uses its handle (ivit_handle), its status codes and every one of its conventions: device pointers, dense
 * row-major tensors, asynchronous on the handle's HIP stream, nothing allocated, nothing synchronised, hipGraph-capturable, IVIT_OK or
 * an error code; a pointer named in an "Alignment:" line is refused with IVIT_ERR_INVALID unless aligned, and a pair named in an
 * "Overlap:" line unless disjoint (ivit_last_error then contains "overlap" and both names), before anything is launched.
 *
 * The definition (ivit_amd/predict.py: gauss_score_reference is the numpy fp64 statement).  The model is four fp32 arrays over the
 * features' integers x (feat8 int8 [N, dim]): Wh [R, dim], t [R], Wc [C, dim], bc [C].
 *   z[r, k] = Wh[k, :] . x[r, :] + t[k]                 k < R
 *   q[r]    = sum_k z[r, k]^2                           fp32 [N]   the squared distance to the pooled mean
 *   s[r, c] = Wc[c, :] . x[r, :] + bc[c]                c < C
 *   best[r] = max_c s[r, c]                             fp32 [N]
 *   cls[r]  = the smallest c with s[r, c] == best[r]    int32 [N]
 *   dist[r] = q[r] - best[r]                            fp32 [N]   the squared Mahalanobis distance to the nearest class mean
 * With Wh = Lambda^-1/2 U^T of the shared covariance, t = -Wh mean, m_c = Wh mean_c + t, Wc[c] = 2 Wh^T m_c and
 * bc[c] = 2 t . m_c - |m_c|^2 (gauss_fit_reference), |z - m_c|^2 = q - s[., c].  A class with bc = -inf (an empty class) is never
 * chosen and makes no NaN; if every class is -inf, cls = 0, best = -inf and dist = +inf.  The model's values are finite otherwise.
 * Arithmetic: the products are exact (the model enters the matrix instruction as three bf16 pieces per float, the int8 features are
 * exact in bf16), the sums are fp32 in one fixed order.  No atomics: q, best, cls and dist hold the same bits for every `splits`,
 * every device and every call.  The exactness of the products assumes that all three pieces of a weight are normal bf16 numbers or
 * zero, which holds for |weight| >= 2^-102 (a piece lies at most 24 binary places below its value, bf16's smallest normal is
 * 2^-126); what a smaller weight's pieces become is the matrix instruction's treatment of denormals and is not pinned.
 *
 * Deliberately not here: the fit; per-class covariances (QDA); relative Mahalanobis; the [N, C] scores themselves; a runner-level
 * entry; fp16 / bf16 models.
 */
#ifndef IVIT_GAUSS_H
#define IVIT_GAUSS_H

#include "ivit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: ivit_gauss_model_bytes, ivit_gauss_prepare, ivit_gauss_workspace_bytes, ivit_gauss_score. */
#define IVIT_GAUSS_VERSION 1

/* ---- e1  the size of the prepared model for this shape, in bytes: host only, no handle, nothing launched.  6 bytes per weight of
 * the R + C table rows (the classes padded to a multiple of 32) and 4 per row.
 * Limits as below: IVIT_ERR_UNSUPPORTED for the dim, IVIT_ERR_INVALID for R, C or a null `bytes`.                                     */
/* Alignment: none: `bytes` is a host pointer. */
/* Overlap: none: nothing on the device is read or written. */
int ivit_gauss_model_bytes(int dim, int R, int C, size_t *bytes);

/* ---- e2  the caller's fp32 model -> the prepared form ivit_gauss_score reads, one launch: every weight as three bf16 pieces in the
 * block order the scorer loads, the classes padded to 32 with zero rows, then t and bc (-inf on the padding).  The model is constant
 * across calls, so this runs once per model and device, not per batch.  `model` depends on dim, R and C only through its contents:
 * score it with the same three.
 * Limits: dim a multiple of 64 in 64 .. 1024: IVIT_ERR_UNSUPPORTED otherwise; R a multiple of 32 in 32 .. dim, 1 <= C <= 65536,
 * model_bytes at least what e1 states, every pointer non-null: IVIT_ERR_INVALID otherwise.                                            */
/* Alignment: Wh, Wc and model 16-byte aligned, t and bc 4-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: model may overlap none of Wh, t, Wc and bc: IVIT_ERR_INVALID, nothing launched. */
int ivit_gauss_prepare(ivit_handle h, const float *Wh, const float *t, const float *Wc, const float *bc, int dim, int R, int C, void *model,
                       size_t model_bytes);

/* ---- e3  the workspace of ivit_gauss_score for this shape and `splits`, in bytes: host only, no handle, nothing launched.  One
 * float per row and whitening tile (R / 32 of them) and 8 bytes per row and part of the table.  splits == 0 sizes it for the library's
 * own choice on ANY device (it assumes the largest part count the choice can give).
 * Limits as below: IVIT_ERR_UNSUPPORTED for the dim, IVIT_ERR_INVALID for N, R, C, splits or a null `bytes`.                          */
/* Alignment: none: `bytes` is a host pointer. */
/* Overlap: none: nothing on the device is read or written. */
int ivit_gauss_workspace_bytes(int64_t N, int dim, int R, int C, int splits, size_t *bytes);

/* ---- e4  q, best, cls and dist by the definition above, WRITTEN (not added to), two launches: the scorer (grid: row blocks of 128 x
 * parts of the table; a wavefront keeps 32 rows register-resident and the table's 32-row tiles stream past through
 * v_mfma_f32_32x32x16_bf16, one float per row and whitening tile, one (value, index) per row and part) and the ordered finish (one
 * thread per row) — csrc/ivit_gauss.h.  `splits`: the parts the table's R / 32 + ceil(C / 32) tiles are cut into, at most that many;
 * 0 for the library's choice — as many as bring the grid to about two workgroups per CU, so a batch of one to 256 rows still covers
 * the device, and one part at 100 000 rows.  The results do not depend on it.
 * Limits: dim a multiple of 64 in 64 .. 1024: IVIT_ERR_UNSUPPORTED otherwise; R a multiple of 32 in 32 .. dim, 1 <= C <= 65536,
 * 1 <= N <= 2^31 - 1, 0 <= splits <= 256, model_bytes at least what e1 and workspace_bytes at least what e3 states for the same
 * arguments, every pointer non-null: IVIT_ERR_INVALID otherwise.  model (as e2 left it for the same dim, R and C) and feat8 are not
 * written.  The workspace's contents are the call's own: nothing is carried from one call to the next.                               */
/* Alignment: model, feat8 and workspace 16-byte aligned, q, best, cls and dist 4-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: workspace, q, best, cls and dist may overlap neither model or feat8 nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_gauss_score(ivit_handle h, const void *model, size_t model_bytes, const int8_t *feat8, int64_t N, int dim, int R, int C, int splits,
                     void *workspace, size_t workspace_bytes, float *q, float *best, int32_t *cls, float *dist);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_GAUSS_H */
