/*
 * ivit_logreg.h — logistic-regression probe: the softmax cross-entropy of a float head over a batch of labelled int8 features and its
 * gradient, fused — what an iterative fit (L-BFGS, gradient descent) evaluates 50 to 200 times.  Sixteenth public header of
 * libivit_hip.so.
 *
 * Why an entry of its own: ivit_probe.h holds the statistics of the ridge probe, one pass and a solve.  The linear-probe number
 * people report for a frozen backbone is multinomial logistic regression, whose every step is a pass over the features: logits, a
 * softmax, and the gradient's two products.  In a tensor library that materialises a [rows, classes] matrix three times per step; here
 * a row keeps four numbers and the matrix is never written.
 *
 * Why a sixteenth header: ivit.h is frozen at IVIT_VERSION 111 and the fourteen headers behind it at their versions (their prototypes
 * and versions are pinned by the binding's tests), so these entries are declared here, under a version of their own.  This header
 * includes ivit.h and uses its handle (ivit_handle), its status codes and every one of its conventions: device pointers, dense
 * row-major tensors, asynchronous on the handle's HIP stream, nothing allocated, nothing synchronised, hipGraph-capturable, IVIT_OK or
 * an error code; a pointer named in an "Alignment:" line is refused with IVIT_ERR_INVALID unless aligned, and a pair named in an
 * "Overlap:" line unless disjoint (ivit_last_error then contains "overlap" and both names), before anything is launched.
 *
 * The definition (ivit_amd/predict.py: logreg_reference is the numpy fp64 statement).  feat8 int8 [N, dim] (x: the integers), labels
 * int32 [N], W fp32 [C, dim], b fp32 [C], x_scale the features' scale:
 *   z[r, c]  = x_scale * (W[c, :] . x[r, :]) + b[c]
 *   a row counts where 0 <= labels[r] < C; every other row contributes nothing, as in ivit_probe_accumulate
 *   loss     fp64 [1]       the SUM over the counted rows of logsumexp(z[r, :]) - z[r, labels[r]]
 *   grad_W   fp32 [C, dim]  the sum over the counted rows of (softmax(z[r, :]) - onehot(labels[r])) (x) x[r, :]
 *   grad_b   fp32 [C]       the sum over the counted rows of softmax(z[r, :]) - onehot(labels[r])
 *   correct  int64 [2]      the counted rows, and those whose argmax of z[r, :] — the smallest index on ties — is the label
 * The outputs are WRITTEN, not added to; the mean, the L2 term and the chain rule of x_scale (d loss / d W of a head that acts on
 * x_scale * x is x_scale * grad_W) belong to the caller.
 * Arithmetic: the products are exact (W and the probabilities enter the matrix instruction as three bf16 pieces each, the int8
 * features are exact in bf16), the sums are fp32, the loss terms are fp32 and their sum fp64.  No atomics: the same inputs, `splits`
 * and device give the same bits on every call.  The exactness of the products assumes that all three pieces of a value are normal
 * bf16 numbers or zero, which holds for |value| >= 2^-102 (a piece lies at most 24 binary places below its value, bf16's smallest
 * normal is 2^-126); what a smaller weight's pieces become is the matrix instruction's treatment of denormals and is not pinned.
 *
 * Deliberately not here: the optimiser (ivit_amd/probe.py: fit_logistic); class weights, label smoothing, sigmoid (multi-label)
 * heads; a gradient with respect to the features; fp16 / bf16 heads; a sharded form (sums of per-rank outputs are the caller's).
 */
#ifndef IVIT_LOGREG_H
#define IVIT_LOGREG_H

#include "ivit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: ivit_logreg_workspace_bytes, ivit_logreg_loss_grad. */
#define IVIT_LOGREG_VERSION 1

/* ---- e1  the workspace of ivit_logreg_loss_grad for this shape and `splits`, in bytes: host only, no handle, nothing launched.  It
 * holds W as bf16 pieces (6 bytes per weight, classes padded to 32), 16 bytes per row, and per part of the rows one fp32
 * [classes padded to 32, dim + 1] partial gradient.  splits == 0 sizes it for the library's own choice on ANY device (it assumes the
 * largest part count the choice can give); a part holds at most 65 536 rows, so there are never fewer than ceil(N / 65536).
 * Limits as below: IVIT_ERR_UNSUPPORTED for the dim, IVIT_ERR_INVALID for N, C, splits or a null `bytes`.                            */
/* Alignment: none: `bytes` is a host pointer. */
/* Overlap: none: nothing on the device is read or written. */
int ivit_logreg_workspace_bytes(int64_t N, int dim, int C, int splits, size_t *bytes);

/* ---- e2  loss, gradient and accuracy by the definition above, four launches: the weight pieces, the row statistics (128 rows per
 * workgroup register-resident, the class table streaming past 32 classes at a time through v_mfma_f32_32x32x16_bf16, an online
 * softmax per row), the gradient (a workgroup per 32 classes and part of the rows; the logits recomputed, p - onehot formed from the
 * row statistics and contracted with the rows from an LDS image) and the ordered reduction of the parts (csrc/ivit_logreg.h).
 * `splits`: the parts of the rows in the gradient pass, 0 for the library's choice, at most 4096.
 * Limits: dim a multiple of 64 in 64 .. 1024: IVIT_ERR_UNSUPPORTED otherwise, and where N is 2^31 or more; 2 <= C <= 65536, N >= 1,
 * N * dim < 2^40, N * C < 2^40, 0 <= splits <= 4096, x_scale finite, workspace_bytes at least what e1 states for the same splits, every
 * pointer non-null: IVIT_ERR_INVALID otherwise.  feat8, labels, W and b are not written.  The workspace's contents are the call's own:
 * nothing is carried from one call to the next.                                                                                      */
/* Alignment: feat8, W, grad_W and workspace 16-byte aligned, loss and correct 8-byte, labels, b and grad_b 4-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: workspace, loss, grad_W, grad_b and correct may overlap neither feat8, labels, W or b nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_logreg_loss_grad(ivit_handle h, const int8_t *feat8, const int32_t *labels, int64_t N, int dim, const float *W, const float *b, int C,
                          float x_scale, int splits, void *workspace, size_t workspace_bytes, double *loss, float *grad_W, float *grad_b,
                          int64_t *correct);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_LOGREG_H */
