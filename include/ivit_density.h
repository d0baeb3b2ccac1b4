/*
 * ivit_density.h — density clustering (DBSCAN) over int8 rows, exact, on the device: which rows form dense groups, which are isolated,
 * and how many groups there are, from a threshold and a count instead of a K.  The threshold clustering of the features the engines
 * produce, beside k-means (ivit_cluster.h) and the range search (ivit_range.h).  Eighteenth public header of libivit_hip.so.
 *
 * Why an entry of its own: the other route to connected groups is the pair list of ivit_range.h and a union-find on the host.  At the
 * thresholds of a density clustering a row has hundreds of neighbours: the pair list is then the [rows, rows] matrix this library
 * never writes, and it crosses to the host before the grouping starts.  Label propagation needs, per row, only the SMALLEST LABEL
 * AMONG ITS NEIGHBOURS: a scan that keeps the scores in registers produces it directly.  Memory is O(rows), no sweep needs the host,
 * and the result is a fixed point that depends neither on the grid, nor on `splits`, nor on how often the host looks.
 *
 * It includes ivit.h and uses its handle, its status codes and every one of its conventions: device pointers, dense row-major
 * tensors, asynchronous on the handle's HIP stream, nothing allocated, nothing synchronised, hipGraph-capturable, IVIT_OK or an error
 * code; a pointer named in an "Alignment:" line is refused with IVIT_ERR_INVALID unless aligned, and a pair named in an "Overlap:"
 * line unless disjoint (ivit_last_error then contains "overlap" and both names), before anything is launched.
 *
 * The definition (ivit_amd/predict.py: dbscan_reference is the numpy statement).  x int8 [rows, dim], weight NULL or float [rows]:
 *   dot[i, j]  = sum_c x[i, c] * x[j, c]                                 exact int32 (dim <= 1024: |dot| <= 2^24)
 *   v{i, j}    = fl32(fl32(fl32(dot) * weight[j]) * weight[i]), i <= j   two fp32 multiplies, nothing contracted: FIRST the weight of the
 *                                                                        LARGER index, then that of the smaller; a NULL weight is both
 *                                                                        multiplies left out.  The value ivit_range_fill gives the pair
 *                                                                        (query = smaller row, gallery = larger), bit for bit, and
 *                                                                        symmetric by construction: the two orientations of the two
 *                                                                        roundings may differ in the last bit, and a neighbour relation
 *                                                                        that is not symmetric has no components
 *   neighbour  v{i, j} >= threshold                                      the IEEE comparison; i == j included where its own value passes
 *   degree[i]  = the number of neighbours of i (itself among them where it passes)
 *   core[i]    = degree[i] >= min_pts
 *   label[i]   core row: the smallest row of its connected component in the graph of core-core neighbour pairs;
 *              other rows with a core neighbour (border rows): the smallest label among their core neighbours;
 *              every other row (noise): -1
 * With weight = ivit_gallery_inv_norms (ivit_search.h) v is the cosine.  With min_pts = 1 every row is core and label is the smallest
 * row of its component of the pair list.  Non-finite weights are OUTSIDE the contract, as in ivit_search.h.
 *
 * The order of work: e2 (degree), e3 (init), e4 (sweep) until it reports changed == 0, the caller swapping label / dirty in and out
 * between sweeps, then e5 (border).  Labels only fall and label[i] <= i always holds, so a tile of 32 rows whose labels the last
 * sweep did not change has already contributed all it can: e4 skips it (neither loaded nor multiplied), which is exact.  The fixed
 * point is unique.  A sweep after convergence skips every tile, writes the same labels and reports changed == 0: a caller may queue
 * several sweeps per synchronisation at almost no cost.
 *
 * Deliberately not here: HDBSCAN / OPTICS; an L2 eps; host-resident or multi-chunk rows; a sharded form; a half-work symmetric form
 * with vector atomics; compaction of the core rows; a runner-level entry.
 */
#ifndef IVIT_DENSITY_H
#define IVIT_DENSITY_H

#include "ivit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: ivit_density_workspace_bytes, ivit_density_degree, ivit_density_init, ivit_density_sweep, ivit_density_border. */
#define IVIT_DENSITY_VERSION 1

/* ---- e1  bytes of workspace e2, e4 and e5 need for these arguments: for S parts of the rows (`splits`, or the library's choice for
 * splits == 0: from rows and the handle's CU share AS IT IS AT THIS CALL — ask again after ivit_set_cu_share; never more parts than
 * tiles of 32 rows) the rows * S int32 partial results, the rows int32 minima of a sweep and one byte per tile.  A host query: nothing
 * is launched.  The limits of e2 on rows, dim and splits apply; a null bytes is IVIT_ERR_INVALID.  NO RESULT DEPENDS ON splits.      */
/* Alignment: none (bytes is a host pointer). */
/* Overlap: none. */
int ivit_density_workspace_bytes(ivit_handle h, int64_t rows, int dim, int splits, size_t *bytes);

/* ---- e2  x int8 [rows, dim], weight NULL or float [rows] -> degree int32 [rows] by the definition above.  Two launches
 * (csrc/ivit_density.h): the scan — grid (tiles of 128 rows) x (parts of the same rows, whole tiles of 32), a wavefront's 32 rows
 * register-resident, the rows streamed past them — counts the neighbours of every (row, part), ONE plain store each; a fold adds the
 * parts.  No atomics.
 *   splits   over how many parts the scan runs.  0: the library chooses.  A positive value forces the count (at most 65535, and at
 *            most the number of tiles): a tuning and test switch.  THE RESULT DOES NOT DEPEND ON IT.
 *   limits   rows in 1 .. 2^31 - 1; splits in 0 .. 65535; threshold finite; x, workspace and degree non-null; bytes at least what e1
 *            reports: IVIT_ERR_INVALID otherwise.  dim a multiple of 64 in 64 .. 1024, and a grid below 2^32 work-items (forced splits
 *            on very many rows): IVIT_ERR_UNSUPPORTED otherwise.
 * Everything is checked before anything is launched.  x and weight are not written.                                                   */
/* Alignment: x and workspace 16-byte aligned, degree 4-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: workspace and degree may overlap neither x or weight nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_density_degree(ivit_handle h, const int8_t *x, int64_t rows, int dim, const float *weight, float threshold, int splits, void *workspace,
                        size_t bytes, int32_t *degree);

/* ---- e3  degree int32 [rows] -> label int32 [rows]: i for a core row (degree[i] >= min_pts), INT32_MAX for any other; dirty uint64
 * [ceil(ceil(rows / 32) / 64)]: bit t % 64 of word t / 64 is set where tile t (rows 32 t .. 32 t + 31) holds a core row; the bits
 * behind the last tile are 0.  One launch.  rows in 1 .. 2^31 - 1, min_pts >= 1, non-null pointers: IVIT_ERR_INVALID otherwise.       */
/* Alignment: degree and label 4-byte aligned, dirty 8-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: label and dirty may overlap neither degree nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_density_init(ivit_handle h, const int32_t *degree, int64_t rows, int32_t min_pts, int32_t *label, uint64_t *dirty);

/* ---- e4  one propagation step over the core rows (label_in[q] != INT32_MAX), with the arguments of e2:
 *   m[q]         = min(label_in[q], min of label_in[g] over the neighbours g of q in the tiles dirty_in marks)
 *   label_out[q] = m[m[q]]                                               one pointer jump
 *   dirty_out    the tiles in which label_out differs from label_in (bits behind the last tile 0); changed int32 [1]: their number
 * Rows that are not core keep INT32_MAX.  Four launches: the scan of e2 in its sweep mode (a tile dirty_in does not mark costs neither
 * its loads nor its MFMAs; a wavefront without a core row leaves at once), the fold of the parts into m (workspace), the jump with one
 * byte per tile, and one workgroup that packs the bytes into dirty_out and counts them.  label_in as e3 or an earlier e4 left it (a
 * label that is no row is never followed); the limits of e2.                                                                          */
/* Alignment: x and workspace 16-byte aligned, label_in, label_out and changed 4-byte, dirty_in and dirty_out 8-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: workspace, label_out, dirty_out and changed may overlap neither x, weight, label_in or dirty_in nor each other (the caller ping-pongs label and dirty): IVIT_ERR_INVALID, nothing launched. */
int ivit_density_sweep(ivit_handle h, const int8_t *x, int64_t rows, int dim, const float *weight, float threshold, int splits, void *workspace,
                       size_t bytes, const int32_t *label_in, const uint64_t *dirty_in, int32_t *label_out, uint64_t *dirty_out, int32_t *changed);

/* ---- e5  the labels of the rows that are not core, with the arguments of e2 and the converged label of e4 -> out int32 [rows]: a core
 * row's label is copied; any other row gets the smallest label among its core neighbours, or -1.  Two launches: the scan in its border
 * mode (a wavefront whose 32 rows are all core leaves at once) and the fold.                                                          */
/* Alignment: x and workspace 16-byte aligned, label and out 4-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: workspace and out may overlap neither x, weight or label nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_density_border(ivit_handle h, const int8_t *x, int64_t rows, int dim, const float *weight, float threshold, int splits, void *workspace,
                        size_t bytes, const int32_t *label, int32_t *out);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_DENSITY_H */
