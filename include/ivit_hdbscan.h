/*
 * ivit_hdbscan.h — the device half of HDBSCAN over int8 rows, exact: every row's CORE SIMILARITY (its min_pts-th largest value, itself
 * counted) and the maximum spanning forest of the MUTUAL-REACHABILITY values, about rows - 1 edges.  HDBSCAN needs no K and no
 * threshold and handles clusters of different density and noise; ivit_density.h asks for a threshold, and the single linkage of
 * ivit_linkage.h chains through noise.  Everything behind the forest — the condensed tree, the stabilities, the selection — runs on
 * the host over those edges (ivit_amd/cluster.py: Linkage.condense).  Twentieth public header of libivit_hip.so.
 *
 * Why entries of their own: both halves are passes over all pairs whose scores never leave registers.  ivit_search_topk cannot give
 * the core similarity: its value has ONE weight and is not symmetric, so its bits differ from ivit_density_* and ivit_linkage_*, and it
 * carries 64-bit keys with indices nobody reads here.  The forest is the Borůvka round of ivit_linkage.h with one changed value.
 *
 * It includes ivit_linkage.h (and through it ivit.h) and uses every one of their conventions: device pointers, dense row-major
 * tensors, asynchronous on the handle's HIP stream, nothing allocated, nothing synchronised, hipGraph-capturable, IVIT_OK or an error
 * code; a pointer named in an "Alignment:" line is refused with IVIT_ERR_INVALID unless aligned, and a pair named in an "Overlap:"
 * line unless disjoint (ivit_last_error then contains "overlap" and both names), before anything is launched.
 *
 * The definition (ivit_amd/predict.py: hdbscan_reference is the numpy statement).  x int8 [rows, dim], weight NULL or float [rows]:
 *   v{i, j}    the value of ivit_density.h / ivit_linkage.h, the LARGER row's weight first, a NULL weight both multiplies left out,
 *              -0.0 counted as +0.0 (v + 0.0f) before any use.
 *   core[i]    the min_pts-th largest element of the MULTISET { v{i, j} : j = 0 .. rows - 1 }, j == i included (as
 *              ivit_density_degree counts a row itself), equal values with their multiplicity; min_pts in 1 .. min(rows, 64).  For
 *              every threshold t: ivit_density_degree at t counts at least min_pts rows for row i exactly when core[i] >= t.
 *   m{i, j}    min(v{i, j}, core[i], core[j]) for i != j, the mutual reachability; the minimums are exact.  At min_pts == 1, m == v.
 *   forest     ivit_linkage.h's, word for word, with m in place of v: edges i < j with m >= floor exist, totally ordered by m
 *              descending, then i ascending, then j ascending; the result is the forest Kruskal's algorithm builds.  m ties
 *              massively (many edges of a row equal core[i]); the total order settles every tie.
 * Non-finite weights are OUTSIDE the contract.
 *
 * The order of work: e2 (the core similarities) once, ivit_linkage_init (ivit_linkage.h: the state before the first round is the
 * same, there is no second init), then e3 (a round) until state reports merged == 0 or components == 1.  A round after the end leaves
 * at once in every launch and changes nothing.  The SLOT an edge lands in is unspecified; the SET of edges is the contract.
 *
 * Deliberately not here: GLOSH outlier scores and membership probabilities; cluster_selection_epsilon; prediction for new rows;
 * host-resident or multi-chunk rows; a sharded form; an L2 form; a half-work symmetric scan.
 */
#ifndef IVIT_HDBSCAN_H
#define IVIT_HDBSCAN_H

#include "ivit_linkage.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: ivit_core_workspace_bytes, ivit_core_similarity, ivit_reach_round. */
#define IVIT_HDBSCAN_VERSION 1

/* ---- e1  bytes of workspace e2 needs for these arguments: for S parts of the rows (`splits`, or the library's choice for splits ==
 * 0, as ivit_density_workspace_bytes chooses: ask again after ivit_set_cu_share) the rows * S * min_pts 32-bit ordered values.  A host
 * query: nothing is launched.  The limits of e2 on rows, dim, min_pts and splits apply; a null bytes is IVIT_ERR_INVALID.  NO RESULT
 * DEPENDS ON splits.                                                                                                                  */
/* Alignment: none (bytes is a host pointer). */
/* Overlap: none. */
int ivit_core_workspace_bytes(ivit_handle h, int64_t rows, int dim, int min_pts, int splits, size_t *bytes);

/* ---- e2  core float [rows]: core[i] as defined above, never -0.0.  Two launches (csrc/ivit_hdbscan.h):
 *   scan     ivit_density_degree's geometry — grid (tiles of 128 rows) x (parts of the same rows, whole tiles of 32), a wavefront's 32
 *            rows register-resident, the rows streamed past them through v_mfma_i32_32x32x32_i8 — with a candidate list per row in
 *            LDS: 32-bit ordered values alone, 64 slots for min_pts <= 16 and 128 above, a STRICT filter against the row's running
 *            min_pts-th value (the multiset is what counts: an equal value changes nothing).  Per (row, part) the min_pts best ordered
 *            values go to the workspace, 0-padded.
 *   select   a wavefront per row: the min_pts-th largest of its parts' values WITH multiplicity.
 *   splits   over how many parts the scan runs.  0: the library chooses.  A positive value forces the count (at most 65535, and at
 *            most the number of tiles): a tuning and test switch.  THE RESULT DOES NOT DEPEND ON IT.
 *   limits   rows in 1 .. 2^31 - 1; splits in 0 .. 65535; min_pts in 1 .. min(rows, 64); x, workspace and core non-null; bytes at least
 *            what e1 reports: IVIT_ERR_INVALID otherwise.  dim a multiple of 64 in 64 .. 1024, and a grid below 2^32 work-items:
 *            IVIT_ERR_UNSUPPORTED otherwise.
 * Everything is checked before anything is launched.  x and weight are not written.                                                   */
/* Alignment: x and workspace 16-byte aligned, core 4-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: workspace and core may overlap neither x or weight nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_core_similarity(ivit_handle h, const int8_t *x, int64_t rows, int dim, const float *weight, int min_pts, int splits, void *workspace,
                         size_t bytes, float *core);

/* ---- e3  one Borůvka round over m, in place: ivit_linkage_round with the edge value m{i, j} = min(v{i, j}, core[i], core[j]).  The
 * workspace has the size and layout of ivit_linkage_workspace_bytes and the state before the first round is ivit_linkage_init's:
 * neither has an entry of its own here.  Six launches; fold, pick, hook, jump and finish are those of ivit_linkage_round, unchanged.
 *   scan     ONE source with ivit_linkage_round's.  The tile rows' core values are loaded beside their weights, the resident row's
 *            once.  v is tested against the running best first (v bounds m from above), then m and the floor test on m.  Because
 *            m{q, .} <= core[q] and the walk ascends, a row whose best equals core[q] is settled, and a wavefront all of whose active
 *            rows are settled leaves the walk (one ballot per tile).  No result depends on it.
 *   core     float [rows], read only: any values are taken (the definition above with this array as core); e2 writes the array meant.
 *   splits, limits   as ivit_linkage_round; core non-null: IVIT_ERR_INVALID otherwise.
 * Everything is checked before anything is launched.  x, weight and core are not written.                                             */
/* Alignment: x and workspace 16-byte aligned, core, comp, edge_u, edge_v, edge_val and state 4-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: workspace, comp, done, edge_u, edge_v, edge_val and state may overlap neither x, weight or core nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_reach_round(ivit_handle h, const int8_t *x, int64_t rows, int dim, const float *weight, const float *core, float floor, int splits,
                     void *workspace, size_t bytes, int32_t *comp, uint8_t *done, int32_t *edge_u, int32_t *edge_v, float *edge_val, int32_t *state);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_HDBSCAN_H */
