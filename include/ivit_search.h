/*
 * ivit_search.h — gallery search: the k nearest rows of an int8 gallery for every int8 query, by exact integer dot product or by
 * cosine, from the features the engines already produce (ivit_features.h: "for retrieval, a linear probe, a second head on the same
 * backbone").  Seventh public header of libivit_hip.so.
 *
 * Why an entry of its own: ivit_linear_i8 followed by ivit_logits_topk writes the whole [queries, gallery] int32 score matrix to
 * memory (256 queries against 1.28 M rows: 1.3 GB, beside a 492 MB gallery), rescans a row once per rank above 1 024 columns, stops at
 * k = 16 and takes the gallery in one piece with int counts.  ivit_search_topk streams the gallery ONCE, keeps the scores in registers
 * and emits the k best per query; ivit_search_merge combines the results of several calls, so a gallery may be searched chunk by chunk
 * or rank by rank.
 *
 * Why a seventh header: ivit.h is frozen at IVIT_VERSION 111, ivit_eval.h at IVIT_EVAL_VERSION 1, ivit_features.h at
 * IVIT_FEATURES_VERSION 1, ivit_attnmap.h at IVIT_ATTNMAP_VERSION 1, ivit_classmap.h at IVIT_CLASSMAP_VERSION 1 and ivit_hidden.h at
 * IVIT_HIDDEN_VERSION 1 (their prototypes and versions are pinned by the binding's tests), so these entries are declared here, under a
 * version of their own.  This header includes ivit.h and uses its handle (ivit_handle), its status codes and every one of its
 * conventions: device pointers, dense row-major tensors, asynchronous on the handle's HIP stream, nothing allocated, nothing
 * synchronised, hipGraph-capturable, IVIT_OK or an error code; a pointer named in an "Alignment:" line is refused with
 * IVIT_ERR_INVALID unless aligned, and a pair named in an "Overlap:" line unless disjoint (ivit_last_error then contains "overlap" and
 * both names), before anything is launched.
 *
 * The definition (ivit_amd/predict.py: search_reference and inv_norms_reference are the numpy statements):
 *   dot[b, g] = sum_c query[b, c] * gallery[g, c]        exact int32 (dim <= 1024: |dot| <= 1024 * 128^2 = 2^24)
 *   v[b, g]   = fl32(fl32(dot[b, g]) * weight[g])        one conversion (exact: |dot| <= 2^24), one fp32 multiply, nothing contracted
 *   v[b, g]   = fl32(dot[b, g])                          when weight == NULL
 *   order     that of ivit_logits_topk, word for word: descending by value; -0.0 equal to +0.0; equal values by ascending gallery
 *             index.  Row b of idx is index_base + the first k entries of np.lexsort((arange(rows), -(v[b] + 0.0))); val holds the
 *             bits of v (-0.0 stays -0.0).  Non-finite weights are OUTSIDE the contract.
 *
 * Deliberately not here: approximate indices; float or fp16 galleries; a runner-level graph form (the entries are capturable: a
 * caller's graph can hold them); a sharded-gallery helper (ivit_search_merge is the building block); the query's own norm (a per-row
 * constant: it does not change a query's order).
 */
#ifndef IVIT_SEARCH_H
#define IVIT_SEARCH_H

#include "ivit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: ivit_gallery_inv_norms, ivit_search_workspace_bytes, ivit_search_topk, ivit_search_merge. */
#define IVIT_SEARCH_VERSION 1

/* ---- e1  the cosine weights of a gallery: gallery int8 [rows, dim] -> inv_norm float [rows].  ss[g] = sum_c gallery[g, c]^2 as an
 * exact integer; inv_norm[g] = fl32(1.0 / sqrt((double)ss[g])) with the fp64 root and the fp64 division correctly rounded, one
 * rounding to fp32 behind them; a row of zeros gives +0.0f (the idiom of IVIT_FEATURES_UNIT).  With weight = inv_norm the order of a
 * query's neighbours in e3 is the cosine order (the query's own norm is a per-row constant and is not applied).  rows >= 0 (0: nothing
 * launched), gallery / inv_norm non-null: IVIT_ERR_INVALID otherwise.  dim a multiple of 16 in 16 .. 65536: IVIT_ERR_UNSUPPORTED
 * otherwise.  One launch (csrc/ivit_search.h).                                                                                       */
/* Alignment: gallery 16-byte aligned: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: inv_norm may not overlap gallery: IVIT_ERR_INVALID, nothing launched. */
int ivit_gallery_inv_norms(ivit_handle h, const int8_t *gallery, int64_t rows, int dim, float *inv_norm);

/* ---- e2  bytes of workspace e3 needs for these arguments: nq * S * k * 8, S the number of parts the first phase runs over
 * (`splits`, or the library's choice for splits == 0: from nq, rows and the handle's CU share AS IT IS AT THIS CALL — ask again after
 * ivit_set_cu_share).  A host query: nothing is launched.  The limits of e3 on nq, rows, dim, k and splits apply; a null bytes is
 * IVIT_ERR_INVALID.                                                                                                                   */
/* Alignment: none (bytes is a host pointer). */
/* Overlap: none. */
int ivit_search_workspace_bytes(ivit_handle h, int nq, int64_t rows, int dim, int k, int splits, size_t *bytes);

/* ---- e3  the k best gallery rows of every query: query int8 [nq, dim], gallery int8 [rows, dim], weight NULL or float [rows]
 * (ivit_gallery_inv_norms: cosine) -> idx int32 [nq, k], val NULL or float [nq, k], by the definition above; row g of the gallery is
 * reported as index_base + g.  Two launches (csrc/ivit_search.h): the first streams the gallery once through
 * v_mfma_i32_32x32x32_i8 — grid (parts of the gallery) x (tiles of 128 queries), the queries register-resident — turns every
 * accumulator into a 64-bit key and keeps the k best keys per (query, part) in the workspace; the second selects the k best of a
 * query's S * k keys, one wavefront per query.  No workgroup waits for another.
 *   splits   over how many parts of the gallery the first phase runs.  0: the library chooses.  A positive value forces the count
 *            (at most 65535): a tuning and test switch, as ivit_mlp_plan_select is.  THE RESULT DOES NOT DEPEND ON IT.
 *   limits   1 <= k <= 64 and k <= rows; index_base >= 0 and index_base + rows <= 2^31 - 1; nq >= 0 (0 launches nothing); splits in
 *            0 .. 65535; query, gallery, idx and workspace non-null; bytes at least what e2 reports: IVIT_ERR_INVALID otherwise.
 *            dim a multiple of 64 in 64 .. 1024 (every num_features of the library's models): IVIT_ERR_UNSUPPORTED otherwise.
 * Everything is checked before anything is launched.  query, gallery and weight are not written.                                     */
/* Alignment: query and gallery 16-byte aligned, workspace 8-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: idx, val and workspace may overlap neither query, gallery or weight nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_search_topk(ivit_handle h, const int8_t *query, int nq, const int8_t *gallery, int64_t rows, int dim, const float *weight, int k,
                     int32_t index_base, int splits, void *workspace, size_t bytes, int32_t *idx, float *val);

/* ---- e4  the second phase of e3 made public: the k best of each row's candidates, idx_in int32 [nq, ncand] and val_in float
 * [nq, ncand] -> idx int32 [nq, k], val NULL or float [nq, k], in the same order and from (val, idx) alone: descending by val_in,
 * -0.0 equal to +0.0, equal values by ascending idx_in; val holds the winners' bits.  What lets a caller search a gallery chunk by
 * chunk (each chunk with its index_base) or rank by rank, lay the results side by side and combine them.  Candidate indices must be
 * non-negative and distinct within a row, the values finite: the result is unspecified otherwise (nothing is written out of
 * bounds).  1 <= k <= 64, ncand >= k, nq >= 0 (0 launches nothing), idx_in / val_in / idx non-null: IVIT_ERR_INVALID otherwise.
 * One launch.                                                                                                                        */
/* Alignment: none beyond the elements' own 4 bytes. */
/* Overlap: idx and val may overlap neither idx_in or val_in nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_search_merge(ivit_handle h, const int32_t *idx_in, const float *val_in, int nq, int ncand, int k, int32_t *idx, float *val);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_SEARCH_H */
