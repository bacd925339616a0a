/* sblas_hip_eigsh.h -- a few extremal eigenpairs of a symmetric CSR matrix by thick-restart Lanczos (Wu and Simon) with
 * full reorthogonalisation, on a device plan, its two stand-alone kernels and its host references.
 * Additive: sblas_hip.h includes this file, and every entry point declared there keeps its signature and its bits. */
#ifndef SBLAS_HIP_EIGSH_H
#define SBLAS_HIP_EIGSH_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * For a square CSR matrix with fp64 values and int32 indices that the caller promises to be symmetric (not checked, as
 * with PCG).  k eigenpairs at one end of the spectrum (`which`: the largest, the smallest, the largest in magnitude) from
 * a basis V of ncv + 1 columns: 1 <= k < ncv <= min(64, n - 1), k <= keep <= ncv - 1.
 *   - a step at column j (GMRES's step without M^-1; every dot has sblas_hip_krylov_dot_f64's bits, nothing is fused):
 *       w = A v_j;  h_i = (v_i, w), i <= j;  w = w - h_0 v_0 - ... - h_j v_j, ascending, rounded product and rounded
 *       difference;  c_i = (v_i, w), h_i = h_i + c_i;  w = w - c_0 v_0 - ... - c_j v_j;  beta = sqrt((w, w));
 *       T[i][j] = T[j][i] = h_i for i <= j;  v_{j+1} = w / beta, a rounded division per element.
 *     beta not finite: BREAKDOWN.  beta == 0: an invariant subspace, the cycle ends at j + 1 columns, no further step
 *     acts and the Ritz step ends the solve: CONVERGED when j + 1 >= k, else BREAKDOWN.
 *   - the Ritz step over the mm finished columns (mm = ncv unless the cycle ended early): T = Y diag(theta) Y^T by cyclic
 *     Jacobi.  M = mm rounded up to even, a missing index padded with zeros.  A sweep is M - 1 rounds of M / 2 disjoint
 *     pairs, the circle method with index M - 1 fixed: pair 0 of round r is (r, M - 1), pair i is ((r + i) mod (M - 1),
 *     (r - i) mod (M - 1)), the smaller index p first.  A round takes every pair's rotation from T as the round began:
 *       skipped (c = 1, s = 0) when a_pq == 0 or |a_pp| + |a_pq| == |a_pp| and |a_qq| + |a_pq| == |a_qq|; else
 *       tau = (a_qq - a_pp) / (2 a_pq);  t = sign(tau) / (|tau| + sqrt(1 + tau tau)), or 1 / (2 tau) when |tau| >= 2^500;
 *       c = 1 / sqrt(1 + t t);  s = t c;  a_pp' = a_pp - t a_pq;  a_qq' = a_qq + t a_pq;  a_pq' = 0 (skipped or not).
 *     Then every 2 x 2 block of T at rows (p1, q1) of pair b1 and columns (p2, q2) of pair b2 becomes J1^T B J2 with
 *     J = [c s; -s c], x_p' = c x_p - s x_q, x_q' = s x_p + c x_q: the columns first and then the rows where b1 < b2, the
 *     rows first where b1 > b2 (the same arithmetic transposed, so T stays symmetric to the bit), and every row of Y takes
 *     its pair's column rotation.  The loop ends behind the first sweep without a rotation, or behind sweep 24.
 *     A value of T that is not finite: BREAKDOWN, nothing else changes.
 *   - behind it: the Ritz values in order (LA descending, SA ascending, LM descending |theta|, ties by index);
 *     rho_i = |beta Y[mm-1][i]|; the test rho_i <= max(rtol |theta_i|, atol) on the first k; the restart is counted;
 *     CONVERGED when all k meet it (or the subspace is invariant), else LIMIT at max_restarts, else RUNNING;
 *     Q = the first kk = min(keep, mm) ordered columns of Y; T = diag(theta_0 .. theta_{kk-1}); kk columns are finished.
 *   - the rotation: V[:, i] = Q[0][i] V[:, 0], then + Q[l][i] V[:, l] ascending in l < mm, rounded product and rounded
 *     sum, for i < kk, in place, and column mm moves to column kk: column i has the bits of sblas_hip_gmres_combine_f64 over
 *     V's first mm columns with Q's column i.  It runs behind every Ritz step that acts, the last one included, so V's
 *     first k columns end as the Ritz vectors.
 *   - a single-vector Lanczos method finds ONE copy of a multiple eigenvalue: the k values returned are then not the k
 *     extremal ones counted with multiplicity, however small the residuals (a block method is what that needs).
 * ------------------------------------------------------------------------------------- */
#define SBLAS_EIGSH_MAX_NCV 64
#define SBLAS_EIGSH_BLOCK_SLOTS 16
#define SBLAS_EIGSH_MATRIX_DOUBLES 12560
#define SBLAS_EIGSH_LA 0
#define SBLAS_EIGSH_SA 1
#define SBLAS_EIGSH_LM 2
/* what a breakdown names */
#define SBLAS_EIGSH_DENOM_V0 1        /* |v0| is zero or not finite */
#define SBLAS_EIGSH_DENOM_BETA 2      /* beta of a step is not finite */
#define SBLAS_EIGSH_DENOM_T 3         /* T holds a value that is not finite */
#define SBLAS_EIGSH_DENOM_INVARIANT 4 /* an invariant subspace of fewer than k columns */

/* HOST functions: no GPU call.
 * limits: [0] the largest ncv [1] the default's floor (20) [2] the leading dimension of T, Y, Q [3] the cap on sweeps
 * [4] slots of the scalar block [5] doubles of the small-matrix block, and where in it [6] T [7] Y [8] theta [9] the
 * residual estimates [10] Q [11] h [12] c begin; [13] rows of a rotation workgroup [14] lanes of the Ritz kernel [15] 0.
 * The scalar block, eight-byte slots: [0] status [1] restarts [2] matvecs [3] finished columns [4] beta (double) [5] the
 * breakdown's name [6] the rotation's flag [7] the step's flag [8] rtol [9] atol (doubles) [10] max_restarts [11] how many
 * of the first k met the test [12] invariant [13] mm and [14] kk of the last Ritz step. */
int sblas_eigsh_limits(int64_t out[16]);
/* out = (ncv, keep) with the defaults put in for ncv <= 0 (min(max(2 k + 1, 20), 64, n - 1)) and keep <= 0 (k + (ncv -
 * k) / 2); SBLAS_E_INVALID unless 1 <= k < ncv <= min(64, n - 1) and k <= keep <= ncv - 1 */
int sblas_eigsh_sizes(int64_t n, int k, int ncv, int keep, int64_t out[2]);
/* out: [0] launches of a step (9, an SpMV counted as one) [1] of start (3 + 9 keep) [2] of a cycle (9 (ncv - keep) + 2)
 * [3] of the cycle's Ritz kernel and rotation (2).  Returns [2], or -1. */
int64_t sblas_eigsh_launches(int ncv, int keep, int64_t out[4]);
/* The Jacobi loop on the leading mm x mm of T (by columns, ldt; symmetric, finite): theta[i] = the diagonal it ends with,
 * unordered, Y (by columns, ldy) the eigenvectors by columns; *sweeps (may be NULL): sweeps that rotated. */
int sblas_eigsh_jacobi_ref(int mm, const double *T, int ldt, double *theta, double *Y, int ldy, int *sweeps);
/* The whole Ritz step on host copies of the two blocks, exactly what sblas_hip_eigsh_ritz_f64 does on the device. */
int sblas_eigsh_ritz_ref(int k, int keep, int which, double *blk, double *mat);
/* The scalar part of step j's last fold: T's column j from h, the count, beta's meaning.  1: v_{j+1} is formed; 0: not. */
int sblas_eigsh_step_ref(int j, const double *h, double beta, double *blk, double *mat);
/* The rotation on a host V of mm + 1 columns (column stride ldv): columns 0 .. keep - 1 and column keep are written. */
int sblas_eigsh_rotate_ref(int64_t n, int mm, int keep, double *V, int64_t ldv, const double *Q, int ldq);

/* DEVICE entries that stand alone; stream-ordered, no allocation, no synchronisation.
 * rotate: V has mm + 1 columns of n doubles at stride ldv >= n; Q (device) is mm x keep by columns at stride ldq >= mm,
 * 1 <= keep <= mm <= 64.  One pass: 8 n (mm + 1) bytes read, 8 n (keep + 1) written. */
int sblas_hip_eigsh_rotate_f64(int dev, void *stream, int64_t n, int mm, int keep, double *V, int64_t ldv, const double *Q, int ldq);
/* ritz: blk (16 slots) and mat (SBLAS_EIGSH_MATRIX_DOUBLES doubles) on the device, laid out as above; one workgroup. */
int sblas_hip_eigsh_ritz_f64(int dev, void *stream, int k, int keep, int which, double *blk, double *mat);

/* The plan.  One allocation, zeroed at create: the scalar block, the small-matrix block, the partial sums, V (ncv + 1
 * columns at GMRES's column stride) and w.  ncv <= 0 and keep <= 0 ask for the defaults.  Refused before anything is
 * launched: sizes outside the limits above, an unknown `which`, an SpMV plan made for another structure.  The plan keeps
 * rowptr and colidx (the caller's) and the SpMV plan. */
int sblas_hip_eigsh_plan_create(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx, int k, int ncv,
                                int keep, int which, const void *spmv_plan, uint32_t seed, void **plan_out);
/* Begins a solve: v0 (n doubles on the device, or NULL: sblas_cheby_start_ref's hashed vector with the plan's seed) is
 * normalised (a zero or non-finite |v0| is BREAKDOWN), then the first `keep` steps are enqueued.  rtol, atol >= 0. */
int sblas_hip_eigsh_start(void *plan, void *stream, const double *val, const double *v0, double rtol, double atol, int64_t max_restarts);
/* Enqueues `cycles` restart cycles: steps keep .. ncv - 1, the Ritz kernel, the rotation -- always the same chain, so a
 * captured iterate replays to the eager bits.  Allocates nothing, never synchronises, uses no atomics.  Once the status is
 * not RUNNING nothing the plan owns changes but w. */
int sblas_hip_eigsh_iterate(void *plan, void *stream, int64_t cycles);
/* The one call that synchronises.  out: [0] status (SBLAS_KRYLOV_*) [1] restarts [2] matvecs [3] how many of the first k
 * estimates met the test [4] beta [5] the breakdown's name (SBLAS_EIGSH_DENOM_*) or 0 [6] columns of the last Ritz step
 * [7] finished columns.  theta, residuals: k doubles each on the host (either may be NULL). */
int sblas_hip_eigsh_status(const void *plan, void *stream, double out[8], double *theta, double *residuals);
/* theta's first k values to a device array (a stream-ordered copy) */
int sblas_hip_eigsh_values(const void *plan, void *stream, double *out);
/* V itself: column i of the basis at *V + i * *ldv, n doubles each; the first k columns are the Ritz vectors once the
 * solve has ended.  The plan's own memory: it lives until destroy and the next start overwrites it.  No GPU call. */
int sblas_hip_eigsh_vectors(const void *plan, const double **V, int64_t *ldv);
/* out: [0] n [1] nnz [2] k [3] ncv [4] keep [5] which [6] the column stride of V in bytes [7] bytes of the partials
 * [8] of the scalar block [9] of the small-matrix block [10] bytes on the device [11] launches of a step [12] of start
 * [13] of a cycle */
int sblas_hip_eigsh_info(const void *plan, int64_t out[14]);
int sblas_hip_eigsh_destroy(void *plan);

#ifdef __cplusplus
}
#endif
#endif /* SBLAS_HIP_EIGSH_H */
