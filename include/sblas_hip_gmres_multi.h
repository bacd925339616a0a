/* sblas_hip_gmres_multi.h -- right-preconditioned restarted GMRES(m) for several right-hand sides on one SpMM per Arnoldi
 * step.  Additive: sblas_hip.h includes this file, and every entry point declared there keeps its
 * signature and its bits. */
#ifndef SBLAS_HIP_GMRES_MULTI_H
#define SBLAS_HIP_GMRES_MULTI_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * A X = B with A an n x n CSR matrix (fp64 values, int32 indices), X and B of n rows and s columns, ROW-MAJOR with a
 * leading dimension >= s (sblas_hip_krylov_multi.h's layout).  1 <= s <= SBLAS_GMRES_MULTI_MAX_RHS, 1 <= restart <=
 * SBLAS_GMRES_MULTI_MAX_RESTART.  Batched, not block GMRES: s independent GMRES(m) recurrences that share A and run in
 * lockstep, each column with its own Hessenberg column, Givens rotations, g, R, stopping test, count, restart count,
 * status and bits.  The directions never mix.
 *   - the basis is m + 1 blocks V_0 .. V_m, each n x s row-major with leading dimension s, one block stride apart: the
 *     block the next step multiplies is an SpMM operand without a copy.
 *   - W = A Z is ONE call of sblas_hip_spmm_csr_ordered_f64_i32_planned per step, on a plan for width s the solver plan
 *     owns, both orders SBLAS_ROW_MAJOR, alpha 1 and beta 0.  The solver takes the SpMM's bits as they come.
 *   - a step for column c is the single solver's step (sblas_hip.h's GMRES section) on column c: classical Gram-Schmidt
 *     twice; h_i = (V_i[:, c], W[:, c]) with exactly the bits of the pinned dot on those two strided columns (cells of
 *     2048 rows, lane t the rows t, t + 256, ..., product and sum rounded separately from +0, the butterfly,
 *     (w0 + w1) + (w2 + w3), one workgroup over the cells); the projection ascending, each product and each difference
 *     rounded; eta = sqrt((w, w)); the scalar step -- the single solver's own text (sblas_gmres_step_ref); v = w / eta by
 *     a rounded division; z = v, or the rounded dinv o v with Jacobi.
 *   - close and restart are the single solver's, per column: one lane a column decides whether the close acts (the
 *     column is pending and its cycle is full or its status is not RUNNING) and back-substitutes; u = y_0 v_0, then
 *     u = u + y_l v_l ascending; z = M^-1 u; x = x + z.  A restart forms r = b - A x through the SpMM, tests the true
 *     residual and is counted.  A close sits behind every m-th step and at the end of every iterate.
 *   - the position is read from the device: no kernel takes the count of finished columns from the launch.  Column c
 *     reads it from scalar block c (16 eight-byte slots, the single solver's layout; block c at scalars + 16 c); its
 *     small-matrix block has the single solver's layout at a fixed stride (limits [7]).  An iterate captured in a graph
 *     replays from any position.
 *   - the freeze, per column.  Once column c is not RUNNING no solver kernel reads, modifies or writes column c of X or
 *     of V, nor its g, R, c, s, count and status -- except the one close that applies its pending columns.  The others go
 *     on.  The product and an applied M^-1 run on whole blocks, frozen columns included, and write work blocks only;
 *     start clears the work blocks first, so a solve's bits depend on its own operands alone.  The solve is over when no
 *     column runs.
 *   - edges per column as in the single solver: b_c = 0 gives x_c = 0, converged at iteration 0; |r0| within the
 *     tolerance leaves x_c untouched; a NaN never converges; max_iter = 0 is LIMIT; a breakdown names
 *     SBLAS_GMRES_DENOM_GIVENS or SBLAS_GMRES_DENOM_BETA and keeps the columns before it; eta = 0 converges without a
 *     division.  n = 0 launches nothing and every column reads converged.
 *   - preconditioners: SBLAS_PRECOND_NONE, SBLAS_PRECOND_JACOBI (one dinv of n entries shared by the columns),
 *     SBLAS_PRECOND_AMG with its plan in lower_plan (the block cycle of sblas_hip_amg_multi.h), SBLAS_PRECOND_ILU0 with
 *     its pair of solve plans (the two tiled solves of sblas_hip_sptrsm_tile.h).  Chebyshev has no multi-column apply
 *     and is refused.
 *   - so a whole solve equals, bit for bit, the lockstep loop composed of that SpMM, the pinned dot per column, numpy
 *     updates, the scalar step and M^-1 on one column.  NOT promised: that column c equals a single-right-hand-side
 *     solve of b_c, or a batch of another width -- the SpMM's row sums have their own order.
 *   - no atomics, nothing waits across workgroups, no cooperative launch, no allocation after create; only status
 *     synchronises; iterate is a linear graph-capturable chain.
 * ------------------------------------------------------------------------------------- */
#define SBLAS_GMRES_MULTI_MAX_RHS 64
#define SBLAS_GMRES_MULTI_TILE 8
#define SBLAS_GMRES_MULTI_MAX_RESTART 64

/* HOST functions (no GPU call; testable alone).  limits: [0] the most right-hand sides [1] columns of a tile [2] cell
 * size [3] lanes of a cell [4] the largest restart [5] blocks beside the m + 1 of the basis (a kind that cannot run in
 * place adds one) [6] slots of a column's scalar block [7] doubles of a column's small-matrix block (their stride). */
int sblas_gmres_multi_limits(int64_t out[8]);
/* Workgroups of one multi-column pass: [0] cells = ceil(n / 2048) [1] tiles = ceil(s / 8) [2] their product, the grid
 * [3] columns of the last tile.  SBLAS_E_INVALID for n < 0 or s outside [1, 64]. */
int sblas_gmres_multi_grid(int64_t n, int nrhs, int64_t out[4]);
/* out: launches of [0] a step [1] a close [2] a restart [3] start -- the single solver's (sblas_gmres_launches) with the
 * SpMV's one launch replaced by spmm_launches, whatever s is.  lower_or_cycle_launches: the block cycle's launches (AMG)
 * or the lower tiled solve's (ILU(0)); upper_launches: the upper solve's; both 0 for NONE and JACOBI.  Returns the
 * launches of a full cycle, m steps, a close and a restart; -1 for a restart outside [1, 64], a kind without a
 * multi-column apply, launches named for a kind that has none, or a negative count. */
int64_t sblas_gmres_multi_launches(int restart, int precond, int64_t spmm_launches, int64_t lower_or_cycle_launches, int64_t upper_launches,
                                   int64_t out[4]);
/* SBLAS_OK when the plan takes this kind alone (NONE, JACOBI) / with one plan in lower_plan (AMG) / with a pair of
 * solve plans (ILU(0)), else SBLAS_E_INVALID. */
int sblas_gmres_multi_precond_ok(int precond);
int sblas_gmres_multi_precond_plan_ok(int precond);
int sblas_gmres_multi_precond_pair_ok(int precond);

/* The kernels alone, on k <= 65 basis blocks: block i is the n x s row-major block at V + i * block_stride with leading
 * dimension ldv.  scalars: NULL, or s device blocks of 16 slots whose slot [0] is a status as int64 -- a column whose
 * status is not SBLAS_KRYLOV_RUNNING is neither read nor written.  Refused, not overrun (SBLAS_E_INVALID): a leading
 * dimension below s, k > 1 with block_stride < n * ldv, an operand that is not 8-byte aligned; a short workspace is
 * SBLAS_E_WORKSPACE.  Operands need 8-byte alignment only: 16-byte accesses are taken when every base and leading
 * dimension allows, with the same bits.  Stream-ordered, allocate nothing, never synchronise, graph-capturable.
 *   dots     out[i * s + c] = (V_i[:, c], W[:, c]) in ONE pass over memory, each with the single pinned dot's bits;
 *            workspace: at least ..._dots_workspace(n, s, k) bytes; stage 1 leaves partial[(i * s + c) * cells + cell].
 *   project  W[:, c] <- W[:, c] - H[c * ldh + 0] V_0[:, c] - H[c * ldh + 1] V_1[:, c] - ..., ascending, each product and
 *            each difference rounded; partial: NULL, or s * cells doubles that take stage 1 of (w, w) over the new W,
 *            column c, cell at partial[c * cells + cell].
 *   combine  U[:, c] = Y[c * ldy + 0] V_0[:, c], then U[:, c] = U[:, c] + Y[c * ldy + l] V_l[:, c] ascending. */
size_t sblas_hip_gmres_multi_dots_workspace(int64_t n, int nrhs, int k);
int sblas_hip_gmres_multi_dots_f64(int dev, void *stream, int64_t n, int nrhs, int k, const double *V, int64_t ldv, int64_t block_stride,
                                   const double *W, int64_t ldw, const double *scalars, double *out, void *workspace, size_t workspace_bytes);
int sblas_hip_gmres_multi_project_f64(int dev, void *stream, int64_t n, int nrhs, int k, const double *V, int64_t ldv, int64_t block_stride,
                                      const double *H, int64_t ldh, double *W, int64_t ldw, const double *scalars, double *partial);
int sblas_hip_gmres_multi_combine_f64(int dev, void *stream, int64_t n, int nrhs, int k, const double *V, int64_t ldv, int64_t block_stride,
                                      const double *Y, int64_t ldy, double *U, int64_t ldu, const double *scalars);

/* The plan.  create makes and owns an SpMM plan for width s on (rowptr, colidx), its workspace, the m + 1 basis blocks
 * and the work blocks (leading dimension s), the partial sums, s scalar blocks and s small-matrix blocks; it may
 * synchronise `stream`, and nothing after it allocates.  precond and its plans: NONE or JACOBI with both plans NULL;
 * AMG with the plan in lower_plan (its level vectors are reserved for s columns here) and upper_plan NULL; ILU0 with the
 * lower and the upper solve plan.  Refused (SBLAS_E_INVALID): s or restart out of range, CHEBYSHEV or an unknown kind,
 * plans missing, surplus, on another device or made for another structure.  A create that cannot get its device memory
 * returns SBLAS_E_HIP and leaks nothing.  The plan keeps the POINTERS rowptr and colidx, which must outlive it. */
int sblas_hip_gmres_multi_plan_create(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx, int nrhs,
                                      int restart, int precond, const void *lower_plan, const void *upper_plan, void **plan_out);
/* out: [0] n [1] nnz [2] restart [3] precond [4] s [5] blocks owned (m + 1 + limits [5], one more for AMG) [6] bytes of
 * one [7] bytes of the partials [8] of the scalar blocks [9] of the small-matrix blocks [10] of the SpMM's workspace
 * [11] device bytes held (the SpMM plan's own apart) [12] launches of a step [13] of a close [14] of a restart [15] of a
 * full cycle, each without the products' (sblas_gmres_multi_launches with spmm_launches 0) */
int sblas_hip_gmres_multi_plan_info(const void *plan, int64_t out[16]);
/* Copies block k of the plan -- 0 .. m: V_k; then W, U, Z -- into out, n x s doubles row-major with leading dimension s on
 * the device, stream-ordered: what a test of the freeze looks at.  SBLAS_E_INVALID for k outside the blocks owned. */
int sblas_hip_gmres_multi_plan_block(const void *plan, void *stream, int k, double *out);
int sblas_hip_gmres_multi_plan_destroy(void *plan);
/* start: clears the work blocks, then per column |b_c|, r_c = b_c - A x_c (A X by the SpMM, then one rounded
 * difference), the test at iteration 0 and v_0.  lu_or_dinv: the inverse diagonal (JACOBI) or the factor (ILU0), else
 * ignored.  X on entry holds the initial guesses and is updated in place as cycles close; it must not overlap B as
 * address ranges (two interleaved column slices of one wider tensor count as overlapping).  ldb, ldx >= s; rtol, atol
 * >= 0 (a NaN is refused), max_iter >= 0 counts Arnoldi steps, the same for every column.  An AMG plan must be set up,
 * with a smoother that has a block form.  Stream-ordered on the calling thread's current device, which must be the
 * plan's; allocates nothing, never synchronises. */
int sblas_hip_gmres_multi_start(void *plan, void *stream, const double *val, const double *lu_or_dinv, const double *B, int64_t ldb, double *X,
                                int64_t ldx, double rtol, double atol, int64_t max_iter);
/* iterate: enqueues k lockstep steps, a close and a restart behind every restart-th, and a close at its end -- a fixed
 * linear chain of launches, no allocation, no synchronisation (graph-capturable).  SBLAS_E_INVALID before start. */
int sblas_hip_gmres_multi_iterate(void *plan, void *stream, int64_t k);
/* status: copies the scalar blocks back and synchronises `stream` -- the only call of a solve that does.  out: s x 8
 * doubles, column c's at out + 8 c in the order of sblas_hip_gmres_status. */
int sblas_hip_gmres_multi_status(const void *plan, void *stream, double *out);

#ifdef __cplusplus
}
#endif
#endif /* SBLAS_HIP_GMRES_MULTI_H */
