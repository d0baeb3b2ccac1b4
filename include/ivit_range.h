/*
 * ivit_range.h — range search: ALL rows of an int8 gallery whose score against an int8 query reaches a threshold, exact, in CSR
 * form; the threshold consumer of the features the engines produce, beside the top-k search (ivit_search.h), the probe
 * (ivit_probe.h) and k-means (ivit_cluster.h).  Twelfth public header of libivit_hip.so.
 *
 * Why an entry of its own: "which rows lie within cosine t of this image" and "which images of this set are near-duplicates of
 * each other" are questions with a threshold, not a k.  ivit_search_topk returns exactly k rows, stops at k = 64, leaves the
 * query's own norm out (a per-row constant does not change an order; it does change a threshold) and knows no "pairs i < j"; the
 * other route, ivit_linear_i8 and a nonzero over the [queries, gallery] int32 matrix, writes the matrix ivit_search.h exists to
 * avoid, and a self-join has as many queries as rows.  Here the gallery is streamed twice through v_mfma_i32_32x32x32_i8, the
 * scores stay in registers, and the variable-length result is deterministic: no atomics, no dependence on the grid, on `splits`
 * or on chunking, every index and every bit of every value those of a numpy statement.
 *
 * Why a twelfth header: the eleven older headers are frozen under their versions (their prototypes are pinned by the binding's
 * tests), so these entries are declared here, under a version of their own.  This header includes ivit.h and uses its handle
 * (ivit_handle), its status codes and every one of its conventions: device pointers, dense row-major tensors, asynchronous on the
 * handle's HIP stream, nothing allocated, nothing synchronised, hipGraph-capturable, IVIT_OK or an error code; a pointer named in
 * an "Alignment:" line is refused with IVIT_ERR_INVALID unless aligned, and a pair named in an "Overlap:" line unless disjoint
 * (ivit_last_error then contains "overlap" and both names), before anything is launched.
 *
 * The definition (ivit_amd/predict.py: range_reference is the numpy statement):
 *   dot[b, g] = sum_c query[b, c] * gallery[g, c]                       exact int32 (dim <= 1024: |dot| <= 2^24)
 *   v[b, g]   = fl32(fl32(fl32(dot[b, g]) * weight[g]) * qweight[b])    two fp32 multiplies in this order, nothing contracted; a NULL
 *                                                                       weight / qweight is that multiply left out
 *   hit[b, g] = v[b, g] >= threshold                                    the IEEE comparison: -0.0 >= +0.0 is a hit
 *               and, if triangle != 0, index_base + g > query_base + b
 *   row b of the result: the hits of query b by ASCENDING g; idx = index_base + g, val = the bits of v (-0.0 stays -0.0)
 *   row_ptr int64 [nq + 1]: row b is idx[row_ptr[b] .. row_ptr[b + 1]); row_ptr[0] = 0, row_ptr[nq] = the total
 * With qweight == NULL v is ivit_search_topk's val bit for bit: a row of the result is then the entries of that search at k = rows
 * whose value is >= threshold, by index.  For the cosine both weights come from ivit_gallery_inv_norms (ivit_search.h), which
 * works on any int8 rows, the queries included; a row of zeros has the weight +0.0 and hence v = +-0.  Non-finite weights are
 * OUTSIDE the contract, as in ivit_search.h.
 *
 * Two passes, the caller between them: ivit_range_count writes row_ptr (and the per-part counts and offsets into the workspace),
 * ivit_range_fill writes idx / val at those offsets.  A caller who must size idx exactly reads row_ptr[nq] between the two (one
 * synchronisation); a caller with a fixed buffer passes its `capacity`, queues or captures both and checks row_ptr[nq] <= capacity
 * afterwards.  Triangle: with query == gallery, query_base == index_base and triangle = 1 the result is every pair i < j once (a
 * self-join at about half the work: tiles wholly at or below the diagonal are not loaded); chunk against chunk with the chunks'
 * bases gives the same pairs in pieces.
 *
 * Deliberately not here: an exact-L2 radius; results ordered by value (sort a row, or use the top-k search); int64 indices; a
 * single-pass unordered form; approximate methods (LSH, IVF); a sharded helper (rows of per-rank results concatenate); a
 * runner-level entry or graph form (the entries are capturable: a caller's graph can hold them).
 */
#ifndef IVIT_RANGE_H
#define IVIT_RANGE_H

#include "ivit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: ivit_range_workspace_bytes, ivit_range_count, ivit_range_fill. */
#define IVIT_RANGE_VERSION 1

/* ---- e1  bytes of workspace e2 and e3 need for these arguments: for S parts of the gallery (`splits`, or the library's choice for
 * splits == 0: from nq, rows and the handle's CU share AS IT IS AT THIS CALL — ask again after ivit_set_cu_share) the nq * S int32
 * counts, their nq * S int64 exclusive offsets and the block sums of the scan between them.  A host query: nothing is launched.  The
 * limits of e2 on nq, rows, dim and splits apply; a null bytes is IVIT_ERR_INVALID.  THE RESULT OF e2 / e3 NEVER DEPENDS ON splits. */
/* Alignment: none (bytes is a host pointer). */
/* Overlap: none. */
int ivit_range_workspace_bytes(ivit_handle h, int nq, int64_t rows, int dim, int splits, size_t *bytes);

/* ---- e2  the first pass: query int8 [nq, dim], gallery int8 [rows, dim], weight NULL or float [rows], qweight NULL or float [nq]
 * -> row_ptr int64 [nq + 1] by the definition above, and in the workspace what e3 needs.  Four launches (csrc/ivit_range.h): the
 * scan — grid (tiles of 128 queries) x (parts of the gallery), the queries register-resident, the gallery streamed once — counts the
 * hits of every (query, part), ONE plain store each; three ordinary launches (block sums, their scan, the add) turn the counts, in
 * query-major order, into int64 exclusive offsets and write row_ptr.  No atomics; no workgroup waits for another.
 *   splits   over how many parts of the gallery the scan runs.  0: the library chooses.  A positive value forces the count (at most
 *            65535): a tuning and test switch.  THE RESULT DOES NOT DEPEND ON IT.
 *   limits   rows >= 1; nq >= 0 (0 launches nothing and writes nothing); index_base >= 0, query_base >= 0, index_base + rows <=
 *            2^31 - 1, query_base + nq <= 2^31 - 1; nq * S <= 2^31 - 1; splits in 0 .. 65535; threshold finite; query, gallery,
 *            workspace and row_ptr non-null; bytes at least what e1 reports: IVIT_ERR_INVALID otherwise.  dim a multiple of 64 in
 *            64 .. 1024 (every num_features of the library's models): IVIT_ERR_UNSUPPORTED otherwise.
 * Everything is checked before anything is launched.  query, gallery, weight and qweight are not written.                           */
/* Alignment: query and gallery 16-byte aligned, workspace and row_ptr 8-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: workspace and row_ptr may overlap neither query, gallery, weight or qweight nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_range_count(ivit_handle h, const int8_t *query, int nq, const int8_t *gallery, int64_t rows, int dim, const float *weight,
                     const float *qweight, float threshold, int32_t index_base, int32_t query_base, int triangle, int splits, void *workspace,
                     size_t bytes, int64_t *row_ptr);

/* ---- e3  the second pass: with the arguments of e2 and the workspace EXACTLY as e2 left it -> idx int32 [capacity], val NULL or float
 * [capacity].  One launch of the same kernel source as e2's scan (the two passes cannot disagree about a hit): the gallery is
 * streamed a second time, and every hit whose position p in the result is < capacity writes idx[p] = index_base + g and, if val is
 * non-null, val[p] = v.  Positions >= capacity are not written; positions >= row_ptr[nq] hold no hit and are not written either.
 * With other arguments than e2's, or a workspace disturbed since, the CONTENT of idx / val is unspecified, but nothing is ever
 * written outside [0, capacity).  capacity >= 0 and idx non-null (whatever the capacity), beside the limits of e2: IVIT_ERR_INVALID
 * otherwise.  query, gallery, weight, qweight and the workspace are not written.                                                     */
/* Alignment: query and gallery 16-byte aligned, workspace 8-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: idx and val may overlap neither query, gallery, weight, qweight or workspace nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_range_fill(ivit_handle h, const int8_t *query, int nq, const int8_t *gallery, int64_t rows, int dim, const float *weight,
                    const float *qweight, float threshold, int32_t index_base, int32_t query_base, int triangle, int splits, void *workspace,
                    size_t bytes, int64_t capacity, int32_t *idx, float *val);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_RANGE_H */
