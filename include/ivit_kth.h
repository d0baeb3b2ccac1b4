/*
 * ivit_kth.h — neighbour order statistics over int8 rows, exact: for every query the value of its k-th nearest row of a gallery, for
 * ANY k up to the row count, and how many rows lie strictly above it.  The k-th-neighbour similarity is the non-parametric novelty
 * score beside the Mahalanobis score of ivit_gauss.h (usually k = 1000 on a large gallery), the core similarity of HDBSCAN at a
 * min_pts beyond 64, and a similarity quantile of a row.  Twenty-first public header of libivit_hip.so.
 *
 * Why entries of their own: ivit_search_topk and ivit_core_similarity keep k candidates per row in LDS and select by swapping, so
 * their k ends at 64 and cannot grow.  This is a different algorithm, radix select on the 32-bit ordered value: the other side is
 * streamed once per 8-bit digit (four times) through the scan all those entries share and counted into a histogram of 256 bins per row
 * in LDS.  The cost does not depend on k, and the [nq, rows] matrix is never written.
 *
 * It includes ivit_hdbscan.h (and through it ivit.h) and uses every one of their conventions: device pointers, dense row-major
 * tensors, asynchronous on the handle's HIP stream, nothing allocated, nothing synchronised, hipGraph-capturable, IVIT_OK or an error
 * code; a pointer named in an "Alignment:" line is refused with IVIT_ERR_INVALID unless aligned, and a pair named in an "Overlap:"
 * line unless disjoint (ivit_last_error then contains "overlap" and both names), before anything is launched.
 *
 * The definition (ivit_amd/predict.py: kth_reference is the numpy statement).  q int8 [nq, dim], x int8 [rows, dim], weight NULL or
 * float [rows], qweight NULL or float [nq], dot[b, g] the exact integer product of q[b] and x[g]:
 *   v[b, g]    self_join == 0: ivit_range.h's value, fl32(fl32(fl32(dot) * weight[g]) * qweight[b]), a NULL array a multiplication by
 *              1.0f.  With a cosine gallery's inverse norms as weight and the queries' as qweight it is the cosine; with a NULL qweight
 *              it is ivit_search_topk's value.
 *              self_join != 0: q must BE x and nq rows; qweight is ignored; the value is that of ivit_density.h / ivit_linkage.h /
 *              ivit_hdbscan.h, the LARGER row's weight first, the row itself included.
 *   kth[b]     the k-th largest element of the MULTISET { v[b, g] + 0.0f : g = 0 .. rows - 1 } (-0.0 counted as +0.0), equal values
 *              with their multiplicity; k in 1 .. rows.  Never -0.0.  For k <= 64: self_join gives ivit_core_similarity's core[b] bit
 *              for bit, the cross form with a NULL qweight ivit_search_topk's val[b, k - 1] (+ 0.0f).
 *   above[b]   the number of rows g with v[b, g] > kth[b]: above[b] < k, and k - above[b] elements of the tie group lie at or before
 *              rank k.
 * Non-finite weights are OUTSIDE the contract.
 *
 * Deliberately not here: a k per query; several ranks per call; a per-query threshold for ivit_range_count; multi-chunk and
 * host-resident galleries; a sharded form; a half-work symmetric self-join; a sampling-based two-pass select.
 */
#ifndef IVIT_KTH_H
#define IVIT_KTH_H

#include "ivit_hdbscan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: ivit_kth_workspace_bytes, ivit_kth_similarity. */
#define IVIT_KTH_VERSION 1

/* ---- e1  bytes of workspace e2 needs for these arguments: for S parts of x (`splits`, or the library's choice for splits == 0: about
 * one workgroup per CU of the handle's share in parts of at least 1024 rows — ask again after ivit_set_cu_share) nq * S * 256 32-bit
 * counts where S > 1, and 0 where S == 1.  A host query: nothing is launched.  The limits of e2 on nq, rows, dim, splits and
 * self_join apply; a null bytes is IVIT_ERR_INVALID.  NO RESULT DEPENDS ON splits.                                                    */
/* Alignment: none (bytes is a host pointer). */
/* Overlap: none. */
int ivit_kth_workspace_bytes(ivit_handle h, int nq, int64_t rows, int dim, int splits, int self_join, size_t *bytes);

/* ---- e2  kth float [nq], above int64 [nq] as defined above (csrc/ivit_kth.h).  Four passes over x, one per 8-bit digit of the
 * ordered value, most significant first; per query a prefix, a count of the values above it and a histogram of the next digit:
 *   S == 1   ONE launch: a wavefront keeps 32 queries register-resident, streams all of x past them through v_mfma_i32_32x32x32_i8
 *            four times and walks its histograms in LDS between the passes; only kth and above are written.
 *   S > 1    per pass a scan launch over grid (128 queries) x (S parts of x, whole tiles of 32 rows) that stores nq * S histograms
 *            to the workspace, and a pick launch, a wavefront per query, that sums them in int64 and chooses the digit: eight
 *            launches.  Between the passes kth and above hold the state.
 *   splits   S.  0: the library chooses.  A positive value forces the count (at most 65535, and at most the number of tiles): a
 *            tuning and test switch.  THE RESULT DOES NOT DEPEND ON IT.
 *   limits   nq in 0 .. 2^31 - 1 (0: nothing is launched); rows in 1 .. 2^31 - 1; splits in 0 .. 65535; k in 1 .. rows; self_join != 0
 *            only with q == x and nq == rows; q, x, kth and above non-null, and workspace where e1 reports more than 0 bytes; bytes
 *            at least what e1 reports: IVIT_ERR_INVALID otherwise.  dim a multiple of 64 in 64 .. 1024, and a grid below 2^32
 *            work-items: IVIT_ERR_UNSUPPORTED otherwise.
 * Everything is checked before anything is launched.  q, x, weight and qweight are not written.                                       */
/* Alignment: q, x and workspace 16-byte aligned, above 8-byte, kth 4-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: workspace, kth and above may overlap neither q, x, weight or qweight nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_kth_similarity(ivit_handle h, const int8_t *q, int nq, const int8_t *x, int64_t rows, int dim, const float *weight, const float *qweight,
                        int64_t k, int self_join, int splits, void *workspace, size_t bytes, float *kth, int64_t *above);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_KTH_H */
