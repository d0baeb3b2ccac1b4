/*
 * ivit_cluster.h — clustering: exact integer k-means (Lloyd) over int8 feature rows with int8 centroids, the unsupervised consumer of
 * the features ivit_features.h produces (codebooks, de-duplication and balancing of a dataset, pseudo-labels, coarse partitions of a
 * gallery).  Eleventh public header of libivit_hip.so.
 *
 * Why entries of their own: ivit_search_topk ranks by dot product or cosine and has no per-row bias for the centroids' norms, and it
 * streams the many-row side; ivit_probe_accumulate drags the Gram matrix along and wants int64 labels.  With int8 rows and int8
 * centroids every quantity of a Lloyd iteration is an exact integer: assignment, per-cluster sums, counts and inertia depend neither
 * on the grid nor on `splits`, the order of summation, the number of ranks or the machine, and the rounded centroid update is an exact
 * integer function of those sums.  The [rows, K] distance matrix is never written.
 *
 * Why an eleventh header: ivit.h is frozen at IVIT_VERSION 111 and the nine headers behind it at their versions 1 (their prototypes and
 * versions are pinned by the binding's tests), so these entries are declared here, under a version of their own.  This header includes
 * ivit.h and uses its handle (ivit_handle), its status codes and every one of its conventions: device pointers, dense row-major
 * tensors, asynchronous on the handle's HIP stream, nothing allocated, nothing synchronised, hipGraph-capturable, IVIT_OK or an error
 * code; a pointer named in an "Alignment:" line is refused with IVIT_ERR_INVALID unless aligned, and a pair named in an "Overlap:"
 * line unless disjoint (ivit_last_error then contains "overlap" and both names), before anything is launched.
 *
 * The definitions (ivit_amd/predict.py: kmeans_assign_reference, kmeans_stats_reference, kmeans_update_reference and kmeans_reference
 * are the numpy statements).  x int8 [rows, dim], cent int8 [K, dim], cnorm[j] = sum_c cent[j, c]^2 (an exact int32: at most 2^24):
 *   score    s[r, j] = 2 dot[r, j] - cnorm[j], dot the exact int32 product; |s| <= 2^26
 *   assign   assign[r] = the smallest j that maximises s[r, j]: the nearest centroid in squared Euclidean distance, ties to the lower
 *            index; dist2[r] = sum_c x[r, c]^2 - s[r, assign[r]], the exact squared distance, 0 <= dist2 <= 2^26
 *   stats    row r takes part iff 0 <= assign[r] < K:  sum[assign[r], :] += x[r, :],  count[assign[r]] += 1,  inertia += dist2[r]
 *   update   for every j with count[j] > 0 and every c:  cent'[j, c] = floor((2 sum[j, c] + count[j]) / (2 count[j])), the mean rounded
 *            half up, exact in int64 and always in -128 .. 127; an empty cluster keeps its centroid; cnorm' is recomputed; `moved` grows
 *            by the number of centroids of which any byte changed
 * Shared limits: dim a multiple of 64 in 64 .. 1024 (every num_features of the library's models): IVIT_ERR_UNSUPPORTED otherwise;
 * 1 <= K <= 16384; rows >= 0 as int64_t (0 launches nothing); every pointer non-null except where NULL is named as allowed:
 * IVIT_ERR_INVALID otherwise.
 *
 * A Lloyd iteration is three launches and no host round trip — assign, accumulate, update — behind the caller's hipMemsetAsync of the
 * statistics: any number of iterations can be queued, or captured in one graph on one stream (no parallel branches).
 * THE INERTIA NEED NOT FALL MONOTONICALLY: the mean is rounded to int8, so the updated centroid is not the exact minimiser of its
 * cluster's squared distances.  The iteration still settles (in practice within a few tens of steps); no caller may rely on a
 * monotone history.
 *
 * Deliberately not here: spherical / cosine k-means (needs a float weight per centroid); float centroids; mini-batch or
 * streaming-forward variants; k-medoids; an IVF index on top (approximate indices stay out of ivit_search.h); a fused assign +
 * accumulate launch; choosing K.
 */
#ifndef IVIT_CLUSTER_H
#define IVIT_CLUSTER_H

#include "ivit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: ivit_kmeans_norms, ivit_kmeans_assign, ivit_kmeans_accumulate, ivit_kmeans_update. */
#define IVIT_CLUSTER_VERSION 1

/* ---- e1  the centroids' norms: cent int8 [K, dim] -> cnorm int32 [K], cnorm[j] = sum_c cent[j, c]^2.  One small launch.  cent is not
 * written.                                                                                                                           */
/* Alignment: cent 16-byte aligned, cnorm 4-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: cnorm may not overlap cent: IVIT_ERR_INVALID, nothing launched. */
int ivit_kmeans_norms(ivit_handle h, const int8_t *cent, int K, int dim, int32_t *cnorm);

/* ---- e2  the assignment, by the definition above: x int8 [rows, dim], cent int8 [K, dim], cnorm int32 [K] (ivit_kmeans_norms or
 * ivit_kmeans_update wrote it) -> assign int32 [rows] and, unless dist2 is NULL, dist2 int32 [rows].  One launch, no workspace: 128
 * rows per workgroup stay in registers as the operands of v_mfma_i32_32x32x32_i8 while the centroid table streams by, 32 centroids at
 * a time; a lane keeps ONE running best (csrc/ivit_cluster.h).  x, cent and cnorm are not written.  One call takes at most
 * (2^24 - 1) * 128 rows (a launch holds fewer than 2^32 work-items): IVIT_ERR_UNSUPPORTED beyond.                                    */
/* Alignment: x and cent 16-byte aligned, cnorm, assign and dist2 4-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: assign and dist2 may overlap neither x, cent or cnorm nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_kmeans_assign(ivit_handle h, const int8_t *x, int64_t rows, int dim, const int8_t *cent, const int32_t *cnorm, int K, int32_t *assign,
                       int32_t *dist2);

/* ---- e3  the statistics of one chunk of rows, by the definition above: x int8 [rows, dim], assign int32 [rows], dist2 int32 [rows]
 * or NULL -> sum int64 [K, dim], count int64 [K], inertia int64 [1].  The entry ADDS into the three buffers and never zeroes them
 * (as ivit_probe_accumulate does): the caller zeroes them once per iteration, streams its chunks through and combines ranks with one
 * integer all-reduce.  An assign value outside 0 .. K - 1 is the "ignore" label: the row contributes to nothing.  With a NULL dist2
 * the inertia is left untouched (a NULL inertia is then allowed too).  One launch: where K * (dim + 1) int32 fit 64 KB a workgroup adds
 * into a zeroed LDS copy and adds its non-zero words into the int64 arrays once per 65 536 rows; otherwise straight 64-bit global
 * atomic adds, a row's consecutive features from consecutive lanes.  The inertia takes one atomic per wavefront.
 *   splits   over how many parts of the rows the launch runs.  0: the library chooses.  A positive value forces the count (at most
 *            65535): a tuning and test switch, as in ivit_probe_accumulate.  THE RESULT DOES NOT DEPEND ON IT.
 * x, assign and dist2 are not written.                                                                                               */
/* Alignment: x 16-byte aligned, assign and dist2 4-byte, sum, count and inertia 8-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: sum, count and inertia may overlap neither x, assign or dist2 nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_kmeans_accumulate(ivit_handle h, const int8_t *x, const int32_t *assign, const int32_t *dist2, int64_t rows, int dim, int K, int splits,
                           int64_t *sum, int64_t *count, int64_t *inertia);

/* ---- e4  the centroid update, by the definition above: sum int64 [K, dim], count int64 [K] -> cent int8 [K, dim] REWRITTEN IN PLACE
 * (that is the entry's definition: cent is both input and output — the centroid of an empty cluster is kept, `moved` compares old and
 * new bytes), cnorm int32 [K] written for every j, moved int64 [1] ADDED into (the caller zeroes it).  count[j] < 0 is outside the
 * contract.  One small launch.  sum and count are not written.                                                                       */
/* Alignment: cent 16-byte aligned, cnorm 4-byte, sum, count and moved 8-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: cent, cnorm and moved may overlap neither sum or count nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_kmeans_update(ivit_handle h, const int64_t *sum, const int64_t *count, int K, int dim, int8_t *cent, int32_t *cnorm, int64_t *moved);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_CLUSTER_H */
