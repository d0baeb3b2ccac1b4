/*
 * ivit_seed.h — k-means++ seeding on the device: exact greedy D^2 sampling over int8 feature rows, the step in front of the Lloyd
 * iterations of ivit_cluster.h.  Fifteenth public header of libivit_hip.so.
 *
 * Why entries of their own: the four entries of ivit_cluster.h start from centroids somebody chose.  Choosing them by D^2 sampling is
 * one pass over the rows per centre — dot products with a handful of candidate rows, a min against the running nearest-seed distance,
 * an exact 64-bit sum — and the centres depend on each other, so on the host it costs a copy of every row and K passes of numpy.  Here
 * the K passes are queued at once: no host round trip between centres, no host draw (the caller passes the random words).
 *
 * Why a fifteenth header: ivit.h is frozen at IVIT_VERSION 111 and the thirteen headers behind it at their versions (their prototypes
 * and versions are pinned by the binding's tests), so these entries are declared here, under a version of their own.  This header
 * includes ivit.h and uses its handle (ivit_handle), its status codes and every one of its conventions: device pointers, dense
 * row-major tensors, asynchronous on the handle's HIP stream, nothing allocated, nothing synchronised, hipGraph-capturable, IVIT_OK or
 * an error code; a pointer named in an "Alignment:" line is refused with IVIT_ERR_INVALID unless aligned, and a pair named in an
 * "Overlap:" line unless disjoint (ivit_last_error then contains "overlap" and both names), before anything is launched.
 *
 * The definition (ivit_amd/predict.py: kmeans_seed_reference is the numpy statement).  x int8 [rows, dim], `first` a row index, draws
 * uint64 [K, trials] (row 0 is not read), d(r, j) = sum_c (x[r, c] - x[j, c])^2, an exact integer below 2^26:
 *   step 0   idx[0] = first, mind[r] = d(r, first), potential[0] = sum_r mind[r] (int64)
 *   step s   (s = 1 .. K - 1) total = potential[s - 1]; for every l < trials
 *              t_l   = (draws[s, l] * total) >> 64, the high half of the 128-bit product: a draw in [0, total) with no float
 *              c_l   = the first row whose running sum of mind exceeds t_l (numpy: searchsorted(cumsum(mind), t_l, side="right")):
 *                      a row with mind == 0 — a chosen centre or a copy of one — can never be drawn
 *              pot_l = sum_r min(mind[r], d(r, c_l))
 *            the winner is the lowest l with the smallest pot_l: idx[s] = c_winner, mind = min(mind, d(., c_winner)),
 *            potential[s] = pot_winner.  trials == 1 is plain k-means++; trials > 1 the greedy form (scikit-learn takes
 *            2 + floor(ln K) trials)
 *   outputs  idx int32 [K], cent = x[idx] int8 [K, dim], cnorm[j] = sum_c cent[j, c]^2 int32 [K] (what ivit_kmeans_assign reads),
 *            potential int64 [K], picked int32 [1]
 *   fewer than K distinct rows: once `total` is 0 after p < K centres, picked = p, idx[p:] = -1, potential[p:] = 0 and cent[p:] and
 *            cnorm[p:] are NOT WRITTEN; every later launch of the call is a no-op on the device.  Otherwise picked = K.
 * Integers throughout: the result depends neither on the grid nor on how the rows are split nor on any order of summation.
 *
 * Deliberately not here: k-means|| (the oversampling variant); seeding across ranks or across host-resident chunks; cosine /
 * spherical seeding; a device form of drawing K rows uniformly; a fused seed-and-assign launch; choosing K.
 */
#ifndef IVIT_SEED_H
#define IVIT_SEED_H

#include "ivit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: ivit_kmeans_seed_workspace_bytes, ivit_kmeans_seed. */
#define IVIT_SEED_VERSION 1

/* ---- e1  the workspace of ivit_kmeans_seed for this shape, in bytes: host only, no handle, nothing launched.  It holds the call's
 * device-side state, one int32 sum of squares and one int32 nearest-seed distance per row and one int64 per (256 rows, candidate).
 * Limits as below: IVIT_ERR_UNSUPPORTED for the dim, IVIT_ERR_INVALID for rows, trials or a null `bytes`.                           */
/* Alignment: none: `bytes` is a host pointer. */
/* Overlap: none: nothing on the device is read or written. */
int ivit_kmeans_seed_workspace_bytes(int64_t rows, int dim, int trials, size_t *bytes);

/* ---- e2  the whole seeding, by the definition above: x int8 [rows, dim], draws uint64 [K, trials] -> cent int8 [K, dim], cnorm int32
 * [K], idx int32 [K], potential int64 [K], picked int32 [1].  One set-up launch, then three launches per centre and no host round trip
 * between centres: the scan streams x once per centre with up to 32 candidate rows resident as one operand of
 * v_mfma_i32_32x32x32_i8 (csrc/ivit_seed.h), the pick chooses the winner and draws, the locate finds the next candidates' rows.
 * Limits: dim a multiple of 64 in 64 .. 1024: IVIT_ERR_UNSUPPORTED otherwise; 1 <= K <= 16384, 1 <= trials <= 32, 1 <= rows < 2^31,
 * 0 <= first < rows, workspace_bytes at least what e1 states, every pointer non-null: IVIT_ERR_INVALID otherwise.  x and draws are
 * not written.  The workspace's contents are the call's own: nothing is carried from one call to the next.                          */
/* Alignment: x, workspace and cent 16-byte aligned, draws and potential 8-byte, cnorm, idx and picked 4-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: workspace, cent, cnorm, idx, potential and picked may overlap neither x or draws nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_kmeans_seed(ivit_handle h, const int8_t *x, int64_t rows, int dim, int K, int trials, int64_t first, const uint64_t *draws, void *workspace,
                     size_t workspace_bytes, int8_t *cent, int32_t *cnorm, int32_t *idx, int64_t *potential, int32_t *picked);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_SEED_H */
