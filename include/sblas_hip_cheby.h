/* sblas_hip_cheby.h -- Chebyshev smoothing on a device eigenvalue estimate: a polynomial in D^-1 A as a
 * preconditioner of its own on a device plan, the estimate of lambda_max(D^-1 A) it stands on, and their host references.
 * Additive: sblas_hip.h includes this file, and every entry point declared there keeps its signature and its bits. */
#ifndef SBLAS_HIP_CHEBY_H
#define SBLAS_HIP_CHEBY_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * For a square CSR matrix with fp64 values, int32 indices, strictly ascending rows and a stored diagonal (ILU(0)'s
 * structure contract).  Every bit is pinned: every product, sum, quotient and difference is rounded on its own, except
 * the one fused multiply-add per stored entry inside a row sum.
 *   - the row sum s_i(x) is the AMG sweep's: G(p) lanes by the stored length p (4 / 16 / 64), lane l the entries l,
 *     l + G, ... with one fma each from +0, folded by the butterfly l ^ 1, l ^ 2, ...; dots are sblas_krylov_dot_ref's.
 *   - dinv_i = 1 / a_ii.  A diagonal that is not finite and > 0 is reported by check(): the least such row.
 *   - the row bound g = max_i (sum_e |a_ie| / a_ii), the sum sequential in stored order from +0, the maximum by `>` from 0.
 *   - the estimate: k steps of Jacobi-preconditioned CG on A x = b0 from x = 0, x never formed.  b0[i] = (2 h(i) + 1)
 *     2^-32 - 1 with h the colouring's priority hash color_priority(i, color_salt(seed + level)).  r = b0, z = dinv o r,
 *     p = z, rho = (r, z); step j: q = A p; pi = (p, q); alpha_j = rho / pi; m = j + 1; (stop when j = k - 1;) r = r -
 *     alpha_j q; z = dinv o r; rho' = (r, z); beta_j = rho' / rho; rho = rho'; p = z + beta_j p.  The recurrence stops
 *     as soon as pi, alpha_j or beta_j is not finite and > 0 (a beta_j that stops it is dropped): a status word on the
 *     device, after which the launches already enqueued return at entry.
 *   - the tridiagonal t_0 = 1 / alpha_0, t_j = 1 / alpha_j + beta_{j-1} / alpha_{j-1}, e2_j = beta_j / (alpha_j alpha_j)
 *     (j < m - 1); its largest eigenvalue by Sturm bisection between max_j t_j and max_j (t_j + sqrt(e2_{j-1}) +
 *     sqrt(e2_j)): at most 64 halvings mid = lo + (hi - lo) / 2, left when mid <= lo or mid >= hi; the Ritz value is hi.
 *   - lambda_max = min(boost * Ritz, g) when m >= 1, g when m = 0; lambda_min = lambda_max / ratio.
 *   - theta = (lambda_max + lambda_min) / 2, delta = (lambda_max - lambda_min) / 2, sigma = theta / delta, rho_0 = 1 /
 *     sigma; c1_0 = 0, c2_0 = 1 / theta; rho_k = 1 / (2 sigma - rho_{k-1}), c1_k = rho_k rho_{k-1}, c2_k = (2 rho_k) / delta.
 *   - a degree-d application is d launches.  Step 0 from zero: d_i = c2_0 (dinv_i b_i), x_i = d_i.  Step 0 from a guess
 *     x: d_i = c2_0 (dinv_i (b_i - s_i(x))), y_i = x_i + d_i.  Step k: t_i = dinv_i (b_i - s_i(x)), d_i = c1_k d_i + c2_k
 *     t_i, y_i = x_i + d_i.  x and y are distinct arrays.
 * ------------------------------------------------------------------------------------- */
/* HOST functions: no GPU call.  limits: [0] the workgroup [1] the largest degree [2] the most estimate steps [3] the
 * default degree [4] the default steps [5] the bisection's halvings [6] the slots of the scalar block [7] 0. */
int sblas_cheby_limits(int64_t out[8]);
/* b0 (n doubles) of (seed, level) */
int sblas_cheby_start_ref(int64_t n, uint32_t seed, uint32_t level, double *b0);
/* The recurrence: alpha, beta (room for `steps` each; alpha_0 .. alpha_{m-1} and beta_0 .. beta_{m-2} written) and *m.
 * *bad_row: a bad structure (SBLAS_E_INVALID), else the least row whose diagonal is not finite and > 0 (reported, not
 * refused), else -1. */
int sblas_cheby_lanczos_ref(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, uint32_t seed, uint32_t level,
                            int steps, double *alpha, double *beta, int64_t *m, int64_t *bad_row);
/* T and its largest eigenvalue from m >= 1 steps.  t (m) and e2 (m - 1) may be NULL. */
int sblas_cheby_ritz_ref(int m, const double *alpha, const double *beta, double *t, double *e2, double *ritz);
int sblas_cheby_rowbound_ref(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, double *g, int64_t *bad_row);
/* min(boost * ritz, g), or g when m = 0 */
double sblas_cheby_lambda_ref(int64_t m, double ritz, double g, double boost);
/* table: 2 * degree doubles (c1_k, c2_k); *lambda_min = lambda_max / ratio */
int sblas_cheby_coef_ref(double lambda_max, double ratio, int degree, double *table, double *lambda_min);
/* y = the degree-`degree` polynomial applied to b: from zero when x is NULL, else from the guess x.  y must be neither
 * b nor x. */
int sblas_cheby_apply_ref(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, const double *table, int degree,
                          const double *b, const double *x, double *y, int64_t *bad_row);

/* The plan.  create is host work (the structure check that names the first bad row, the rows packed as the sweep's
 * launch packs them) and allocates everything: five work vectors, the dot's partial sums and the scalar block with the
 * table.  The plan keeps rowptr and colidx and sweeps on them.  Refused before any launch: degree outside [1, 64],
 * eig_steps outside [1, 64], eig_boost not finite or < 1, eig_ratio not finite or <= 1, a NaN in either. */
int sblas_hip_cheby_plan_create(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx, int degree,
                                int eig_steps, double eig_boost, double eig_ratio, uint32_t seed, void **plan_out, int64_t *bad_row);
/* dinv and g from val; with lambda_max a NaN the estimate (level 0 of the salt), else the caller's lambda_max (finite and
 * > 0) through the same scalar kernel; then the table.  Device only, repeatable, graph-capturable: no allocation, no
 * synchronisation.  The plan keeps val and sweeps on it until the next setup. */
int sblas_hip_cheby_plan_setup(void *plan, void *stream, const double *val, double lambda_max);
/* z = p(D^-1 A) D^-1 r from zero: `degree` launches.  Refused before setup and when z overlaps r. */
int sblas_hip_cheby_plan_apply(const void *plan, void *stream, const double *r, double *z);
/* y = x + p(D^-1 A) D^-1 (b - A x), from the guess x: `degree` launches.  y overlaps neither b nor x. */
int sblas_hip_cheby_plan_smooth(const void *plan, void *stream, const double *b, const double *x, double *y);
/* The one call that synchronises.  out: [0] the least row with a bad diagonal or -1 [1] m [2] the Ritz value (0 when no
 * step finished or lambda_max was given) [3] g [4] lambda_max [5] lambda_min. */
int sblas_hip_cheby_plan_check(const void *plan, void *stream, double out[6]);
/* The recurrence's scalars and the table after a setup, for the tests (synchronises): alpha, beta (64 each), table
 * (2 * degree).  Any may be NULL. */
int sblas_hip_cheby_plan_scalars(const void *plan, void *stream, double *alpha, double *beta, double *table);
/* out: [0] n [1] nnz [2] degree [3] eig_steps [4] four-lane units of a launch [5] launches of one apply (the degree)
 * [6] bytes on the device [7] 1 after a setup [8] launches of a setup that estimates [9] seed [10], [11] 0 */
int sblas_hip_cheby_plan_info(const void *plan, int64_t out[12]);
int sblas_hip_cheby_plan_speaks_for(const void *plan, int dev, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx);
int sblas_hip_cheby_plan_destroy(void *plan);

/* ---------------------------------------------------------------------------------------
 * The polynomial as the AMG plan's smoother (SBLAS_AMG_CHEBYSHEV = 2; additive: plans set up with SBLAS_AMG_JACOBI / _L1
 * allocate nothing new and keep their bits).  In the walk every one of the nu smoothings is one polynomial of `degree`
 * launches: the pre-smoothing's first from zero, every other one from the current iterate; the coarsest level runs one
 * polynomial of degree coarse_sweeps (<= 64) from zero.  A cycle is (levels - 1) (2 nu degree + 3) + coarse_sweeps launches.
 * After a level's values are assembled that level's estimate runs on the device with the salt seed + level; wd holds
 * 1 / a_ii and the table is the level's own.  omega must be 0 (unset).  A level's direction vector, scalar block and partial
 * sums, and the estimate's four work vectors (sized by level 0, shared by the levels) are allocated by the first such setup
 * of a plan, which is refused (SBLAS_E_INVALID) while the stream is capturing; later setups allocate nothing.
 * ------------------------------------------------------------------------------------- */
int sblas_hip_amg_plan_setup_ex(void *plan, void *stream, const double *val, int smoother, double omega, int nu, int coarse_sweeps,
                                double coarse_scale, int degree, int eig_steps, double eig_boost, double eig_ratio);
/* Level `level`'s estimate after a Chebyshev setup (synchronises).  out: [0] m [1] the Ritz value [2] g [3] lambda_max;
 * table (may be NULL): room for 2 * 64 doubles, *entries (may be NULL) pairs written. */
int sblas_hip_amg_plan_eig(const void *plan, void *stream, int level, double out[4], double *table, int *entries);
/* HOST: launches of one cycle with the polynomial, or -1 */
int64_t sblas_amg_launches_cheb(int levels, int nu, int coarse_sweeps, int degree);
/* HOST: sblas_amg_cycle_ref and sblas_amg_cycle_sa_ref with the polynomial: wd[l] holds 1 / a_ii, table[l] level l's
 * (c1_k, c2_k) pairs (degree of them, coarse_sweeps on the coarsest).  degree 0 is the sweeps' cycle (table unread). */
int sblas_amg_cycle_cheb_ref(int levels, const int64_t *n, const int32_t *const *rowptr, const int32_t *const *colidx,
                             const double *const *val, const double *const *wd, const double *const *table, const int32_t *const *agg,
                             const int32_t *const *aggptr, const int32_t *const *members, int nu, int degree, int coarse_sweeps,
                             double coarse_scale, const double *r, double *z);
int sblas_amg_cycle_cheb_sa_ref(int levels, const int64_t *n, const int32_t *const *rowptr, const int32_t *const *colidx,
                                const double *const *val, const double *const *wd, const double *const *table,
                                const int32_t *const *p_rowptr, const int32_t *const *p_colidx, const double *const *p_val,
                                const int32_t *const *r_rowptr, const int32_t *const *r_colidx, const double *const *r_val, int nu,
                                int degree, int coarse_sweeps, double coarse_scale, const double *r, double *z);

#ifdef __cplusplus
}
#endif
#endif /* SBLAS_HIP_CHEBY_H */
