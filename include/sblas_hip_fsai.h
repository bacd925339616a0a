/* sblas_hip_fsai.h -- FSAI, the factorised sparse approximate inverse of Kolotilina and Yeremin, as a preconditioner on a
 * device plan: a sparse lower-triangular G with G A G^T ~ I for a symmetric positive definite A, applied
 * as z = G^T (G r) by two planned SpMVs, and its host references.
 * Additive: sblas_hip.h includes this file, and every entry point declared there keeps its signature and its bits. */
#ifndef SBLAS_HIP_FSAI_H
#define SBLAS_HIP_FSAI_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * For a square CSR matrix with fp64 values, int32 indices, strictly ascending rows and a stored diagonal (ILU(0)'s
 * structure contract and its refusal, which names the first bad row).  A is taken as symmetric: only entries with
 * column <= row are ever read.
 *   - the pattern of G.  Row i holds the stored entries of A's row i with column <= i, or those of the caller's pattern
 *     (rowptr_g, colidx_g): its rows ascend strictly, entries with column > i are ignored, a row without its diagonal is
 *     refused and named, and it may name positions A does not store (the lower triangle of A^2 is the case it exists
 *     for).  J_i: row i's columns, ascending, m_i of them, the last one i.  A row with m_i > 64 is refused and named unless
 *     max_row = k, 1 <= k <= 64: then every row longer than k keeps its diagonal and the k - 1 entries of largest column
 *     below it.  That thinning is structural and crude: it knows no value, and on a pattern with far neighbours (A^2 of a
 *     grid) it drops the far ones first.  The pattern depends on the structure only.
 *   - the values of row i, every product, difference, quotient and square root rounded on its own (nothing fused):
 *       M[p][q] = A[J[p]][J[q]] for q <= p, read from row J[p] of A, +0.0 where that row stores no such column;
 *       for k = 0 .. m - 1:  d = M[k][k]; unless d is finite and > 0 the row FAILS; c = sqrt(d); M[k][k] = c;
 *                            M[p][k] = M[p][k] / c for p > k;  M[p][q] = M[p][q] - M[p][k] * M[q][k] for k < q <= p;
 *       g[m-1] = 1 / M[m-1][m-1], t = 0;  for q = m - 1 down to 1:  t[p] = t[p] + M[q][p] * g[q] for every p < q, then
 *                            g[q-1] = (-t[q-1]) / M[q-1][q-1].
 *     g solves C^T g = e_m: the FSAI row scaled so that (G A G^T)_ii = 1.  A failed row is its diagonal alone: g_ii = 1 /
 *     sqrt(a_ii) when a_ii is finite and > 0, else 1.0, every other entry +0.0; check() reports the least failed row.
 *   - apply: t = G r is sblas_hip_spmv_csr_f64_i32_planned on G's CSR and z = G^T t sblas_hip_spmv_csr_t_f64_i32_planned
 *     on a transpose plan of G: bit for bit those two calls composed.
 * ------------------------------------------------------------------------------------- */
/* HOST functions: no GPU call.  limits: [0] the workgroup [1] the longest row of G (FSAI_ROW_MAX) [2] the longest row of
 * 4 lanes [3] of 16 lanes [4] doubles of LDS a lane for the triangle [5] for the vector [6] LDS bytes of a workgroup [7] 0 */
int sblas_fsai_limits(int64_t out[8]);
/* G's pattern from A's structure (rowptr_g NULL, nnz_g 0) or from the caller's pattern, thinned to max_row (0: a row
 * above 64 entries is refused).  out_rowptr: n + 1 entries; out_colidx: room for the source's entries (A's or the
 * pattern's), out_rowptr[n] of them written; NULL counts only.  *bad_row: the first row that is refused -- by ILU(0)'s
 * check of A, a pattern row that does not ascend or leaves [0, n), a row without its diagonal, a row too long -- else -1. */
int sblas_fsai_pattern(int64_t n, const int32_t *rowptr, const int32_t *colidx, int64_t nnz_g, const int32_t *rowptr_g, const int32_t *colidx_g,
                       int max_row, int32_t *out_rowptr, int32_t *out_colidx, int64_t *bad_row);
/* G's values by the scalar loop above, on the pattern sblas_fsai_pattern gave.  *bad_row: a bad structure of A
 * (SBLAS_E_INVALID), else the least failed row (reported, not refused), else -1. */
int sblas_fsai_ref(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, const int32_t *rowptr_g, const int32_t *colidx_g,
                   double *val_g, int64_t *bad_row);

/* The kind under the Krylov and GMRES plans: the plan's handle in lower_plan's place, upper_plan NULL.  5 stays no kind. */
#define SBLAS_PRECOND_FSAI 6

/* The plan.  create is host work: the structure (and the caller's pattern) comes to the host once, sblas_fsai_pattern
 * checks it and gives G's pattern, which is uploaded.  The plan owns G's structure and values, the temporary t, an SpMV
 * plan on G and a transpose plan on G with its SpMV plan; it keeps rowptr and colidx (A's) and gathers from them.
 * rowptr_g NULL (with nnz_g 0 and colidx_g NULL): A's lower part.  max_row 0: refuse a row above 64. */
int sblas_hip_fsai_plan_create(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx, int64_t nnz_g,
                               const int32_t *rowptr_g, const int32_t *colidx_g, int max_row, void **plan_out, int64_t *bad_row);
/* G's values from val: ONE launch of the gather-and-Cholesky kernel, then the transpose plan's value update.  Device
 * only, repeatable, graph-capturable: no allocation, no synchronisation. */
int sblas_hip_fsai_plan_setup(void *plan, void *stream, const double *val);
/* z = G^T (G r): two planned SpMVs.  Refused before a setup and when z overlaps r.  Allocates nothing, graph-capturable. */
int sblas_hip_fsai_plan_apply(const void *plan, void *stream, const double *r, double *z);
/* The one call that synchronises.  *bad_row: the least row the last setup failed, or -1. */
int sblas_hip_fsai_plan_check(const void *plan, void *stream, int64_t *bad_row);
/* G's device arrays (any output may be NULL): rowptr (n + 1), colidx and val (info's [2]); they live until destroy */
int sblas_hip_fsai_plan_csr(const void *plan, const int32_t **rowptr_g, const int32_t **colidx_g, const double **val_g);
/* out: [0] n [1] nnz [2] nnz of G [3] the longest row of G [4] four-lane units of the setup launch [5] launches of one
 * apply (2: an SpMV counts as the solvers' rule counts it) [6] bytes on the device [7] 1 after a setup [8] rows of 4
 * lanes [9] of 16 lanes [10] of 64 lanes [11] 0 */
int sblas_hip_fsai_plan_info(const void *plan, int64_t out[12]);
int sblas_hip_fsai_plan_speaks_for(const void *plan, int dev, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx);
int sblas_hip_fsai_plan_destroy(void *plan);

#ifdef __cplusplus
}
#endif
#endif /* SBLAS_HIP_FSAI_H */
