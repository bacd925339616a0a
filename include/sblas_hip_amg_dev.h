/* sblas_hip_amg_dev.h -- the AMG plan's aggregation on the device: the pinned rule of sblas_amg_aggregate
 * in Jones-Plassmann rounds, its synchronous host reference, the stand-alone device aggregation and the create that uses
 * it.  Additive: sblas_hip.h includes this file, and every entry point declared there or in sblas_hip_amg_sa.h keeps its
 * signature and its bits. */
#ifndef SBLAS_HIP_AMG_DEV_H
#define SBLAS_HIP_AMG_DEV_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * The rule in round form.  h(u) = the colouring's priority with the salt of (seed + level), as in sblas_amg_aggregate.
 * A vertex v is decided by the states of the strong neighbours u of ITS OWN ROW with h(u) > h(v) (strength is not
 * symmetric: only row v is consulted):
 *   - v is a non-root as soon as one such u is a root;
 *   - v is a root once all such u are decided non-roots (at once when there is no such u);
 *   - otherwise v waits.
 * A state is final once written, so whatever the schedule the fixed point is the greedy walk of sblas_amg_aggregate in
 * descending h.  The aggregates then follow from the roots alone: roots numbered in ascending vertex index, every other
 * vertex with the first root among ALL its strong neighbours in stored order, members by (aggregate, vertex).
 * ------------------------------------------------------------------------------------- */
#define SBLAS_AMG_AGG_HOST 0   /* create aggregates every level on the host (sblas_hip_amg_plan_create[_ex]) */
#define SBLAS_AMG_AGG_DEVICE 1 /* create aggregates every level on the device */

/* HOST function: the synchronous form -- every round reads only the states of the rounds before it.  The arguments and
 * refusals of sblas_amg_aggregate.  root_out: n bytes, 1 for a root.  *rounds: the rounds that decided a vertex (0 for
 * n = 0), the upper bound of the device's. */
int sblas_amg_roots_rounds_ref(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, double theta,
                               uint32_t seed, uint32_t level, unsigned char *root_out, int64_t *rounds, int64_t *bad_row);

/* One level's aggregation on DEVICE arrays: agg, aggptr, members and *n_agg equal sblas_amg_aggregate's, integer for
 * integer.  val NULL: structure only, theta must be 0.  agg, members: n; aggptr: room for n + 1 (n_agg + 1 are written).
 * The structure contract is sblas_amg_aggregate's (strictly ascending rows, a stored diagonal, rowptr[n] == nnz) and is
 * NOT re-checked here.  The call allocates nothing, synchronises `stream` (it reads the round counters and n_agg) and
 * refuses before any launch: theta outside [0, 1] or NaN, theta > 0 without val, n or nnz beyond INT_MAX, a workspace
 * that is missing, short (SBLAS_E_WORKSPACE) or not 16-byte aligned.  *rounds: the rounds that decided a vertex, at
 * most sblas_amg_roots_rounds_ref's; how far below is not part of the contract.  A round that decides nothing while
 * vertices remain is SBLAS_E_INTERNAL. */
size_t sblas_hip_amg_aggregate_workspace(int64_t n, int64_t nnz);
int sblas_hip_amg_aggregate_i32(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                                const double *val, double theta, uint32_t seed, uint32_t level, int32_t *agg, int32_t *aggptr,
                                int32_t *members, void *workspace, size_t workspace_bytes, int64_t *n_agg, int64_t *rounds);

/* sblas_hip_amg_plan_create_ex with the aggregation mode.  SBLAS_AMG_AGG_HOST is create_ex itself.  With
 * SBLAS_AMG_AGG_DEVICE the plan is the same plan, array for array: level 0's structure still comes to the host once for
 * the check that names the first bad row; every level is aggregated by sblas_hip_amg_aggregate_i32, the triplets of the
 * coarse pattern (or of P) are written by a kernel, with theta > 0 the next level's values are the COO plan's assembly on
 * the device, and below level 0 only row pointers and scalars come to the host.  A bad mode is SBLAS_E_INVALID.
 * sblas_hip_amg_plan_options reports the mode in out[3]. */
int sblas_hip_amg_plan_create_dev(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                                  const double *val, double theta, int64_t coarse_max, int max_levels, uint32_t seed,
                                  int prolongator, double prolong_omega, double min_reduction, int aggregation, void **plan_out,
                                  int64_t *bad_row);

#ifdef __cplusplus
}
#endif
#endif /* SBLAS_HIP_AMG_DEV_H */
