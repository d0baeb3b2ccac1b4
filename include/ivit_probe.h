/*
 * ivit_probe.h — linear probe: the exact integer statistics of labelled int8 features from which a least-squares (ridge) head on a
 * frozen backbone is fitted, accumulated in ONE pass over the training images (ivit_features.h: "for retrieval, a linear probe, a
 * second head on the same backbone").  Ninth public header of libivit_hip.so.
 *
 * Why an entry of its own: the ridge probe needs three statistics of the training features and nothing else — the Gram matrix X^T X,
 * the per-class sums and the class counts.  They are integers, exact in int64 under any order of summation, so no feature is ever
 * stored (ImageNet's 1.28 M x 384 features never exist: the state is dim^2 + C dim + C 64-bit words), ranks combine with an integer
 * all-reduce, and the result is pinned bit for bit.  The solve is a dim x dim fp64 system on the host (ivit_amd/probe.py: fit), the
 * way back into an engine is engine.with_head.  The Gram matrix contracts over ROWS while memory is contiguous along the features:
 * the kernel transposes in registers on the way into LDS (csrc/ivit_probe.h).
 *
 * Why a ninth header: ivit.h is frozen at IVIT_VERSION 111 and the seven headers behind it at their versions 1 (their prototypes and
 * versions are pinned by the binding's tests), so this entry is declared here, under a version of its own.  This header includes
 * ivit.h and uses its handle (ivit_handle), its status codes and every one of its conventions: device pointers, dense row-major
 * tensors, asynchronous on the handle's HIP stream, nothing allocated, nothing synchronised, hipGraph-capturable, IVIT_OK or an error
 * code; a pointer named in an "Alignment:" line is refused with IVIT_ERR_INVALID unless aligned, and a pair named in an "Overlap:"
 * line unless disjoint (ivit_last_error then contains "overlap" and both names), before anything is launched.
 *
 * The definition (ivit_amd/predict.py: probe_stats_reference is the numpy statement).  Row r takes part iff 0 <= labels[r] <
 * num_classes, compared as int64:
 *   gram[i, j]              += sum_r x[r, i] * x[r, j]      all i, j: the full symmetric [dim, dim] matrix, both triangles written
 *   class_sum[labels[r], :] += x[r, :]
 *   count[labels[r]]        += 1
 *
 * Deliberately not here: logistic regression or any iterative fit; fine-tuning below the head; several heads in one engine; a
 * runner-level graph form (the entry is capturable: a caller's graph can hold it); choosing the ridge by cross-validation (the
 * statistics are kept, so a caller refits cheaply).
 */
#ifndef IVIT_PROBE_H
#define IVIT_PROBE_H

#include "ivit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: ivit_probe_accumulate. */
#define IVIT_PROBE_VERSION 1

/* ---- e1  the statistics of one batch, by the definition above: feat8 int8 [rows, dim], labels int64 [rows] -> gram int64
 * [dim, dim], class_sum int64 [num_classes, dim], count int64 [num_classes].  The entry ADDS into the three buffers and never zeroes
 * them: the caller zeroes them once and streams its batches through.  A row whose label lies outside 0 .. num_classes - 1 contributes
 * to nothing, not even to gram: it is the "ignore" label (all 64 bits are compared: 2^32 + 3 is not class 3).  The sums are exact,
 * so the result depends neither on `splits` nor on any order; overflow of the int64 totals (beyond 2^49 rows) is outside the
 * contract.  Two launches (csrc/ivit_probe.h): the Gram matrix through v_mfma_i32_32x32x32_i8 — grid (pairs of 128-feature blocks of
 * the upper triangle) x (parts of the rows), int32 accumulators widened to int64 every 65 536 rows — and the class sums and counts;
 * sums of different workgroups meet in 64-bit atomic adds.  No workspace, no workgroup waits for another.
 *   splits   over how many parts of the rows either launch runs.  0: the library chooses.  A positive value forces the count (at
 *            most 65535): a tuning and test switch, as in ivit_search_topk.  THE RESULT DOES NOT DEPEND ON IT.
 *   limits   rows >= 0 (0 launches nothing); 1 <= num_classes <= 65536; splits in 0 .. 65535; feat8, labels, gram, class_sum and count
 *            non-null: IVIT_ERR_INVALID otherwise.  dim a multiple of 64 in 64 .. 1024 (every num_features of the library's models):
 *            IVIT_ERR_UNSUPPORTED otherwise.
 * Everything is checked before anything is launched.  feat8 and labels are not written.                                              */
/* Alignment: feat8 16-byte aligned, labels, gram, class_sum and count 8-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: gram, class_sum and count may overlap neither feat8 or labels nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_probe_accumulate(ivit_handle h, const int8_t *feat8, const int64_t *labels, int64_t rows, int dim, int num_classes, int splits,
                          int64_t *gram, int64_t *class_sum, int64_t *count);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_PROBE_H */
