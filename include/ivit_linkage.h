/*
 * ivit_linkage.h — the single-linkage hierarchy of int8 rows, exact, on the device: the maximum-similarity spanning forest, about
 * rows - 1 edges.  Cutting it at ANY threshold t gives exactly the connected components of the graph v >= t — the groups of
 * ivit_density.h at min_pts = 1 and of the pair list of ivit_range.h — so one computation answers every threshold at once: the tool
 * for choosing the threshold the de-duplication and the density clustering ask for.  Nineteenth public header of libivit_hip.so.
 *
 * Why an entry of its own: a host linkage needs the [rows, rows] matrix this library never writes.  Borůvka's algorithm needs, per
 * round and row, only the BEST NEIGHBOUR OUTSIDE THE ROW'S COMPONENT: a scan that keeps the scores in registers produces it directly.
 * Memory is O(rows), at most ceil(log2 rows) rounds merge anything, and the result depends neither on the grid, nor on `splits`, nor
 * on how often the host looks.
 *
 * It includes ivit.h and uses its handle, its status codes and every one of its conventions: device pointers, dense row-major
 * tensors, asynchronous on the handle's HIP stream, nothing allocated, nothing synchronised, hipGraph-capturable, IVIT_OK or an error
 * code; a pointer named in an "Alignment:" line is refused with IVIT_ERR_INVALID unless aligned, and a pair named in an "Overlap:"
 * line unless disjoint (ivit_last_error then contains "overlap" and both names), before anything is launched.
 *
 * The definition (ivit_amd/predict.py: linkage_reference is the numpy statement).  x int8 [rows, dim], weight NULL or float [rows]:
 *   v{i, j}    the value of ivit_density.h: fl32(fl32(fl32(dot) * weight[j]) * weight[i]) for i < j, the LARGER row's weight first, a
 *              NULL weight both multiplies left out; symmetric, and bit for bit the value ivit_range_fill gives the pair.  A value of
 *              -0.0 counts as +0.0, in the order (as in ivit_logits_topk's) and in edge_val.
 *   edge       an unordered pair i < j.  Edges are TOTALLY ordered: v descending, then i ascending, then j ascending.
 *   floor      a float, -infinity allowed, NaN refused: only edges with v >= floor (the IEEE comparison) exist.
 *   result     the spanning forest Kruskal's algorithm builds: it takes the edges in that order and keeps an edge when it joins two
 *              components.  The order is total, so the forest is unique; with floor = -infinity it is a tree of rows - 1 edges.
 * With weight = ivit_gallery_inv_norms (ivit_search.h) v is the cosine.  Non-finite weights are OUTSIDE the contract.
 *
 * The order of work: e2 (init) once, then e3 (a round) until state reports merged == 0 or components == 1.  A round after the end
 * leaves at once in every launch and changes nothing, so a caller may queue several rounds per read of `state`, or
 * ceil(log2 rows) + 1 of them into one hipGraph and never look.  The SLOT an edge lands in is unspecified (it is the id of the
 * component that hooked with it); the SET of edges is the contract.
 *
 * Deliberately not here: mutual-reachability distances and the condensed tree (HDBSCAN proper); complete or average linkage; an L2
 * form; host-resident or multi-chunk rows; a sharded form; rows sorted by component to skip tiles; a runner-level entry.
 */
#ifndef IVIT_LINKAGE_H
#define IVIT_LINKAGE_H

#include "ivit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: ivit_linkage_workspace_bytes, ivit_linkage_init, ivit_linkage_round. */
#define IVIT_LINKAGE_VERSION 1

/* ---- e1  bytes of workspace e3 needs for these arguments: for S parts of the rows (`splits`, or the library's choice for splits ==
 * 0, as ivit_density_workspace_bytes chooses: ask again after ivit_set_cu_share) the rows * S 64-bit partial keys, and per row a
 * 64-bit key, a 64-bit edge, a 32-bit value and a 32-bit parent.  A host query: nothing is launched.  The limits of e3 on rows, dim
 * and splits apply; a null bytes is IVIT_ERR_INVALID.  NO RESULT DEPENDS ON splits.                                                  */
/* Alignment: none (bytes is a host pointer). */
/* Overlap: none. */
int ivit_linkage_workspace_bytes(ivit_handle h, int64_t rows, int dim, int splits, size_t *bytes);

/* ---- e2  the state before the first round.  comp int32 [rows]: comp[i] = i, every row a component named by itself; done uint8
 * [rows]: 0; edge_u, edge_v int32 [rows] and edge_val float [rows]: every slot -1, -1, 0.0f; state int32 [4]: components = rows,
 * merged = 1, rounds = 0 and a spare word the rounds use.  One launch.  rows in 1 .. 2^31 - 1 and non-null pointers: IVIT_ERR_INVALID
 * otherwise.                                                                                                                          */
/* Alignment: comp, edge_u, edge_v, edge_val and state 4-byte aligned: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: comp, done, edge_u, edge_v, edge_val and state may not overlap each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_linkage_init(ivit_handle h, int64_t rows, int32_t *comp, uint8_t *done, int32_t *edge_u, int32_t *edge_v, float *edge_val, int32_t *state);

/* ---- e3  one Borůvka round, in place.  comp holds a member row of every row's component (which member is not part of the contract).
 * Six launches (csrc/ivit_linkage.h):
 *   scan     grid (tiles of 128 rows) x (parts of the same rows, whole tiles of 32), a wavefront's 32 rows register-resident, the rows
 *            streamed past them through v_mfma_i32_32x32x32_i8: per (row, part) the best edge to a row of ANOTHER component with v >=
 *            floor, as one 64-bit key (ordered value, smallest row), ONE plain store each.  Rows of a done component are skipped.
 *   fold     a thread per row: the best key of its parts; its value into the maximum of the row's component (integer atomicMax).
 *   pick     a thread per row that attains that maximum: its edge into the minimum of the component (integer atomicMin): the
 *            component's best edge under the full edge order.  Both atomics are order-independent: the bits do not depend on scheduling.
 *   hook     a thread per component c: parent[c] = the component of the edge's far end; where two components chose each other the
 *            smaller id stays root; a component without an edge becomes done (its outgoing edges can never change: exact).  A
 *            component that hooks writes its edge into SLOT c of edge_u (the smaller row), edge_v (the larger) and edge_val, and
 *            stops existing: every slot is written at most once in a run, the final roots' slots stay -1, -1, 0.0f.
 *   jump     a thread per row: comp follows parent to its root.
 *   finish   state: components falls by the number of hooks, merged becomes that number, rounds rises by one where anything hooked.
 * When state.merged == 0 on entry every launch leaves at once: no output byte changes, rounds included.
 *   splits   over how many parts the scan runs.  0: the library chooses.  A positive value forces the count (at most 65535, and at
 *            most the number of tiles): a tuning and test switch.  THE RESULT DOES NOT DEPEND ON IT.
 *   limits   rows in 1 .. 2^31 - 1; splits in 0 .. 65535; floor not NaN; every pointer but weight non-null; bytes at least what e1
 *            reports: IVIT_ERR_INVALID otherwise.  dim a multiple of 64 in 64 .. 1024, and a grid below 2^32 work-items (forced splits
 *            on very many rows): IVIT_ERR_UNSUPPORTED otherwise.
 * Everything is checked before anything is launched.  x and weight are not written.                                                   */
/* Alignment: x and workspace 16-byte aligned, comp, edge_u, edge_v, edge_val and state 4-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: workspace, comp, done, edge_u, edge_v, edge_val and state may overlap neither x or weight nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_linkage_round(ivit_handle h, const int8_t *x, int64_t rows, int dim, const float *weight, float floor, int splits, void *workspace,
                       size_t bytes, int32_t *comp, uint8_t *done, int32_t *edge_u, int32_t *edge_v, float *edge_val, int32_t *state);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_LINKAGE_H */
