/* sblas_hip_amg_sa.h -- smoothed aggregation on the AMG plan of sblas_hip.h: prolongator smoothing, the
 * coarsening guard, their host references and the entry points that reach them.  Additive: sblas_hip.h includes this file,
 * and every entry point declared there keeps its signature and its bits. */
#ifndef SBLAS_HIP_AMG_SA_H
#define SBLAS_HIP_AMG_SA_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * Smoothed aggregation on the same plan (additive: a plan made by sblas_hip_amg_plan_create behaves as before).  The
 * rule of a level, every bit pinned:
 *   - the tentative aggregates are level l's sblas_amg_aggregate, unchanged (same seed, theta, level salt); on coarse
 *     levels it runs on the smoothed coarse matrix's structure, and with theta > 0 on its values: create runs the
 *     numeric chain below once on the device with the val given and reads the coarse values back, and the hierarchy is
 *     then fixed as in the plain plan.
 *   - the coarsening guard: the level is kept only when n_next < n and (double)n_next <= (1 - min_reduction) * (double)n,
 *     the product rounded once (sblas_amg_keep_level); with min_reduction 0 any reduction keeps it.  Decided after the
 *     aggregation and before any transfer operator or product is built.
 *   - the prolongator's pattern is the COO plan (SBLAS_COO_SUM) of the triplets (row(e), agg[col(e)]) for e in A_l's
 *     stored order, n_l rows by n_{l+1} columns: strictly ascending rows, and row i stores agg[i].
 *   - its values: q_i = omega_P / a_ii, a rounded division; t_e = -(q_i * a_ie) off the diagonal (a rounded product,
 *     negated) and 1 - q_i * a_ii on it (a rounded product, then a rounded difference, no fma); val_P is the COO plan's
 *     re-assembly of t: duplicates added left to right in input order.  A is used unfiltered, also when theta > 0.
 *     omega_P defaults to 2/3, which is 4 / (3 rho) with rho(D^-1 A) taken as 2: there is no eigenvalue estimate.
 *   - R_l = P_l^T by the device transpose, sblas_hip_csr_transpose_f64_i32: row I lists the fine rows ascending; its
 *     values are gathered through the transpose's perm.
 *   - A_{l+1} = R_l * (A_l * P_l), two SpGEMM plans under that section's contract (S) / (V).
 *   - the transfers in a cycle are one rectangular row product in the sweep's order: s_i over the stored row i of M by
 *     G(p) lanes, lane l the entries l, l + G, ... with one fma each from +0, folded by the butterfly.  Restriction:
 *     b_{l+1}[I] = s_I with M = R_l on the residual.  Prolongation: x_i = x_i + coarse_scale * s_i with M = P_l on the
 *     coarse iterate, a rounded product and a rounded sum, in place.  The walk and the launch count are unchanged.
 * ------------------------------------------------------------------------------------- */
#define SBLAS_AMG_PLAIN 0
#define SBLAS_AMG_SMOOTHED 1
#define SBLAS_AMG_RESTRICT 0 /* modes of sblas_amg_transfer_ref */
#define SBLAS_AMG_PROLONG 1
/* HOST functions.  keep_level: 1 when the guard keeps the level, 0 when it discards it, -1 for a bad argument (n or
 * n_next negative, min_reduction outside [0, 1) or NaN). */
int sblas_amg_keep_level(int64_t n, int64_t n_next, double min_reduction);
/* P's CSR and values from (A, agg, omega_P) in the pinned order.  p_rowptr: n + 1; p_colidx, p_val: room for rowptr[n]
 * entries (either may be NULL to count only), *p_nnz written.  agg[i] in [0, n_agg).  *bad_row: a row without a
 * diagonal (SBLAS_E_INVALID). */
int sblas_amg_prolongator_ref(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, const int32_t *agg,
                              int64_t n_agg, double prolong_omega, int32_t *p_rowptr, int32_t *p_colidx, double *p_val,
                              int64_t *p_nnz, int64_t *bad_row);
/* The row product in lane order over a CSR of `rows` rows.  SBLAS_AMG_RESTRICT: out[i] = s_i (scale unread);
 * SBLAS_AMG_PROLONG: out[i] = out[i] + scale * s_i.  out must not be in. */
int sblas_amg_transfer_ref(int mode, int64_t rows, const int32_t *rowptr, const int32_t *colidx, const double *val, double scale,
                           const double *in, double *out);
/* The walk with general P and R: arrays of `levels` pointers, of which levels - 1 of the p_ and r_ ones are read (P_l has
 * n[l] rows, R_l has n[l + 1]).  z must not be r. */
int sblas_amg_cycle_sa_ref(int levels, const int64_t *n, const int32_t *const *rowptr, const int32_t *const *colidx,
                           const double *const *val, const double *const *wd, const int32_t *const *p_rowptr,
                           const int32_t *const *p_colidx, const double *const *p_val, const int32_t *const *r_rowptr,
                           const int32_t *const *r_colidx, const double *const *r_val, int nu, int coarse_sweeps,
                           double coarse_scale, const double *r, double *z);
/* create with a prolongator (SBLAS_AMG_PLAIN / _SMOOTHED), omega_P (read by a smoothed plan only; fixed here and used
 * by every setup) and the guard.  sblas_hip_amg_plan_create is this with (SBLAS_AMG_PLAIN, unused, 0).  Refused before
 * any launch, beyond create's refusals: a bad prolongator, a smoothed plan's omega_P that is not finite and > 0,
 * min_reduction outside [0, 1) or NaN.  A product whose nnz reaches 2^31 is SBLAS_E_INVALID, with no plan. */
int sblas_hip_amg_plan_create_ex(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                                 const double *val, double theta, int64_t coarse_max, int max_levels, uint32_t seed,
                                 int prolongator, double prolong_omega, double min_reduction, void **plan_out,
                                 int64_t *bad_row);
/* A smoothed plan's transfer operators between level `level` and the next.  sizes: [0] rows of P (n_l) [1] rows of R
 * (n_{l+1}) [2] the stored entries of P, and of R.  ptrs: P's rowptr, colidx, val; R's rowptr, colidx, val (the values
 * are there after a setup).  Refused on a plain plan and on the coarsest level. */
int sblas_hip_amg_plan_transfer(const void *plan, int level, int64_t sizes[3], const void *ptrs[6]);
/* out: [0] the prolongator [1] omega_P (0 on a plain plan) [2] min_reduction [3] the aggregation mode
 * (SBLAS_AMG_AGG_*, sblas_hip_amg_dev.h; 0 for every plan made by the creates above) */
int sblas_hip_amg_plan_options(const void *plan, double out[4]);
/* The prolongator-values kernel alone on level `level` of a smoothed plan: t (the level's nnz) from val; one launch. */
int sblas_hip_amg_pvalues_f64(const void *plan, void *stream, int level, const double *val, double *t);

#ifdef __cplusplus
}
#endif
#endif /* SBLAS_HIP_AMG_SA_H */
