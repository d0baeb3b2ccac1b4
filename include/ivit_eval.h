/*
 * ivit_eval.h — the scoring half of the reference's validate() (quant_train.py:314-351) for a host without torch: per image, the
 * rank of the label among the model's outputs and the cross-entropy of the label.  Second public header of libivit_hip.so.
 *
 * Why a second header: ivit.h is frozen at IVIT_VERSION 111 (its prototypes, structs and version are pinned by the binding's
 * tests), so entries that come after it are declared here, under a version of their own.  This header includes ivit.h and uses its
 * handles (ivit_handle, ivit_vit, ivit_swin, ivit_graph), its status codes and every one of its conventions: device pointers
 * unless a name ends in _host, dense row-major tensors, asynchronous on the handle's HIP stream, nothing allocated, nothing
 * synchronised, hipGraph-capturable, IVIT_OK or an error code.  None of the entries below has an alignment requirement beyond the
 * element type of its pointers.
 *
 * What it replaces (quant_train.py:335-339):
 *   :335  loss = criterion(output, target)                       criterion = nn.CrossEntropyLoss()
 *   :338  prec1, prec5 = accuracy(output, target, topk=(1, 5))   label among the first j outputs  <=>  rank < j
 *   :339  losses.update(loss.data.item(), data.size(0))          mean of nll over the images seen
 */
#ifndef IVIT_EVAL_H
#define IVIT_EVAL_H

#include "ivit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: ivit_logits_score, ivit_vit_score, ivit_swin_score, ivit_vit_score_graph_create, ivit_swin_score_graph_create. */
#define IVIT_EVAL_VERSION 1

/* ---- e1  score: rank and negative log-likelihood of the label, per image.
 * The output is that of ivit_logits_topk (ivit.h, a13), one int -> fp32 conversion (RNE) and one multiply, nothing contracted:
 *   v[b, c] = fl32(fl32(logits[b, c]) * scale[c])
 * logits int32 [batch, num_classes], scale float [num_classes], labels int64 [batch] (what torch carries) ->
 * rank int32 [batch], nll double [batch].  Either output may be NULL, not both.
 *   rank[b]  the number of classes that come strictly before labels[b] in the ORDER of ivit_logits_topk: descending by value, -0.0
 *            and +0.0 equal, equal values by ascending class index.  So idx[b, rank[b]] == labels[b] for the idx of
 *            ivit_logits_topk whenever rank[b] < k, and the label is among the first j outputs exactly when rank[b] < j, for
 *            every j (no limit of 16).  Exact.
 *   nll[b]   with d = (double)v[b, :] and m = max(d): log(sum_c exp(d[c] - m)) - (d[labels[b]] - m), with exp, log and the sum in
 *            fp64 — F.cross_entropy(v.double(), labels, reduction = "none").  The order of the sum is not part of the contract:
 *            two implementations differ by at most (num_classes + 16) * 2^-53 * max(1, |nll|).  The mean over the images is
 *            the reference's `Loss` (torch computes it in fp32: 1e-7 relative from this one).
 * A label outside [0, num_classes) gives rank = INT32_MAX and nll = NaN, and no address is formed from it: it never counts as a
 * hit, and the loss of a set that holds one is NaN (the reference raises there).  Non-finite scale entries are OUTSIDE the
 * contract, as for ivit_logits_topk.
 * batch >= 0, num_classes >= 1, logits, scale, labels and one of rank / nll required: IVIT_ERR_INVALID otherwise (nothing launched).
 * One launch that reads every logits row once (csrc/ivit_score.h).                                                                 */
int ivit_logits_score(ivit_handle h, const int32_t *logits, const float *scale, const int64_t *labels, int batch, int num_classes,
                      int32_t *rank, double *nll);
/* validate()'s `output = model(data)`, `criterion(output, target)` and `accuracy(output, target, ...)` (quant_train.py:334-338) as
 * one call: ivit_vit_forward / ivit_swin_forward of the same arguments (logits is written, with the same integers), then
 * ivit_logits_score of those logits with `head_scale` (float [num_classes], device: "head.scale" of the constants blob) and
 * `labels` (int64 [batch], device) on the handle's stream, behind the slices' join.  head_scale, labels and rank / nll are checked
 * before anything is launched.  The *_graph_create forms capture both (replay: ivit_graph_launch); a replay reads the label
 * buffer again, as it reads the image buffer again.                                                                               */
int ivit_vit_score(ivit_vit m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits,
                   const float *head_scale, const int64_t *labels, int32_t *rank, double *nll);
int ivit_swin_score(ivit_swin m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits,
                    const float *head_scale, const int64_t *labels, int32_t *rank, double *nll);
int ivit_vit_score_graph_create(ivit_vit m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes,
                                int32_t *logits, const float *head_scale, const int64_t *labels, int32_t *rank, double *nll,
                                ivit_graph *out);
int ivit_swin_score_graph_create(ivit_swin m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes,
                                 int32_t *logits, const float *head_scale, const int64_t *labels, int32_t *rank, double *nll,
                                 ivit_graph *out);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_EVAL_H */
