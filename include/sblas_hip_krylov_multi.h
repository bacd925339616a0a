/* sblas_hip_krylov_multi.h -- PCG and BiCGStab for several right-hand sides on one SpMM per product.
 * Additive: sblas_hip.h includes this file, and every entry point declared there keeps its signature and its bits. */
#ifndef SBLAS_HIP_KRYLOV_MULTI_H
#define SBLAS_HIP_KRYLOV_MULTI_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * A X = B with A an n x n CSR matrix (fp64 values, int32 indices) and X, B of n rows and s columns, ROW-MAJOR with a
 * leading dimension >= s: X[i * ldx + j], the layout of a contiguous torch (n, s) tensor or of a column slice of a
 * wider one, which the SpMM's staging copy takes without a transpose.  1 <= s <= SBLAS_KRYLOV_MULTI_MAX_RHS.
 * This is batched solving: s independent recurrences that share A and run in lockstep, each column with its own
 * scalars, stopping test and bits.  It is not block CG: the directions never mix.
 *   - methods SBLAS_KRYLOV_PCG and SBLAS_KRYLOV_BICGSTAB; preconditioners SBLAS_PRECOND_NONE and SBLAS_PRECOND_JACOBI
 *     (one dinv vector of n entries, shared by the columns).  ILU(0), AMG and Chebyshev are refused at create
 *     (SBLAS_E_INVALID): Chebyshev has no multi-column apply, AMG's -- the block cycle of sblas_hip_amg_multi.h -- needs
 *     its plan, which sblas_hip_krylov_multi_plan_create_ex there takes, and ILU(0)'s -- the two tiled solves of
 *     sblas_hip_sptrsm_tile.h -- needs its pair of solve plans, which the create declared there takes.
 *   - A X is one call of sblas_hip_spmm_csr_ordered_f64_i32_planned per product, on a plan for width s the solver plan
 *     owns, both orders SBLAS_ROW_MAJOR, alpha 1 and beta 0.  PCG makes one such call an iteration, BiCGStab two.  The
 *     solver takes the SpMM's bits as they come.
 *   - a column's dot has exactly the bits of the pinned dot (sblas_hip.h's Krylov section) on that strided column:
 *     cells of 2048 rows, lane t of 256 the rows t, t + 256, ..., product and sum rounded separately, the butterfly,
 *     then one workgroup over the cells' sums.  sblas_krylov_dot_ref on the host column is the reference.
 *   - the updates and the scalar step are those of sblas_hip.h's Krylov section, column by column, each with column j's
 *     own alpha, beta, omega from scalar block j (16 eight-byte slots, the single solver's layout; block j at
 *     scalars + 16 j).  The scalar step is the single solver's own text (sblas_krylov_scalar_step_ref compiles it for
 *     the host).
 *   - so a whole solve equals, bit for bit, the lockstep loop composed of that SpMM, the pinned dot per column and the
 *     updates as numpy expressions.  NOT promised: that column j's bits equal a single-right-hand-side solve of b_j, or
 *     a batch of another width -- the SpMM's row sums have their own order, and a plan for another width may select
 *     other kernels.
 *   - the freeze, per column.  Once column j's status is not RUNNING no update reads, modifies or writes column j of
 *     any vector and column j's scalar step changes nothing; the other columns go on.  The SpMM still multiplies the
 *     frozen column of the direction block, into work blocks only.  The solve is over when no column is running.
 *   - edges, per column, as in the single solver: b_j = 0 gives x_j = 0, converged at iteration 0; |r0| within the
 *     tolerance gives converged at 0 with x_j untouched; a NaN never converges; max_iter = 0 is LIMIT at 0 unless
 *     converged.  n = 0 launches nothing and every column reads converged.
 *   - no atomics, nothing waits across workgroups, no cooperative launch, and the host passes no scalar of the
 *     recurrence.
 * ------------------------------------------------------------------------------------- */
#define SBLAS_KRYLOV_MULTI_MAX_RHS 64
#define SBLAS_KRYLOV_MULTI_TILE 8 /* columns of one workgroup: eight consecutive doubles of a row per lane */
/* the scalar steps (sblas_krylov_scalar_step_ref's op), in the order a solve meets them */
#define SBLAS_KRYLOV_STEP_START_B 1    /* d[0] = (b, b): |b|, the tolerance, the block's first state (flag: BiCGStab) */
#define SBLAS_KRYLOV_STEP_START_R 2    /* d[0] = (r0, r0), d[nd - 1] = rho: |r0| and the test at iteration 0          */
#define SBLAS_KRYLOV_STEP_RHO0 3       /* rho = d[0]                                                                  */
#define SBLAS_KRYLOV_STEP_PCG_ALPHA 4  /* alpha = rho / d[0], d[0] = (p, q)                                           */
#define SBLAS_KRYLOV_STEP_PCG_RES 5    /* d[0] = (r, r): |r|, count, test; flag: then beta = d[nd - 1] / rho          */
#define SBLAS_KRYLOV_STEP_PCG_BETA 6   /* beta = d[0] / rho                                                           */
#define SBLAS_KRYLOV_STEP_BICG_ALPHA 7 /* alpha = rho / d[0], d[0] = (r^, v)                                          */
#define SBLAS_KRYLOV_STEP_BICG_OMEGA 8 /* omega = d[0] / d[1]: (t, s), (t, t); d[2] = (s, s) for the half step         */
#define SBLAS_KRYLOV_STEP_BICG_RES 9   /* d[0] = (r, r), d[1] = (r^, r): |r|, count, test, beta                       */

/* HOST functions (no GPU call; testable alone).  limits: [0] the most right-hand sides [1] columns of a tile [2] cell
 * size [3] lanes of a cell [4] work blocks of PCG [5] of BiCGStab (without Jacobi: 3 and 6 of them are touched) [6] dots
 * of one pass [7] slots of a column's scalar block. */
int sblas_krylov_multi_limits(int64_t out[8]);
/* SBLAS_OK when a multi-right-hand-side plan takes this preconditioner kind (none, Jacobi), else SBLAS_E_INVALID */
int sblas_krylov_multi_precond_ok(int precond);
/* Launches of ONE iteration with a product of spmm_launches launches: PCG spmm + 5 (the dots' first stage, fold, x / r
 * update, fold, p update), BiCGStab 2 spmm + 8.  -1 for a bad method, a refused preconditioner or spmm_launches < 0. */
int64_t sblas_krylov_multi_launches(int method, int precond, int64_t spmm_launches);
/* Workgroups of one multi-column pass: [0] cells = ceil(n / 2048) [1] tiles = ceil(s / 8) [2] their product, the grid
 * [3] columns of the last tile.  SBLAS_E_INVALID for n < 0 or s outside [1, 64]. */
int sblas_krylov_multi_grid(int64_t n, int nrhs, int64_t out[4]);
/* The single and the multi solver's scalar step on a HOST block of 16 slots: the text the device folds run.  op: one
 * of SBLAS_KRYLOV_STEP_*; d: nd <= 3 folded sums; rtol, atol, max_iter are read by START_B alone.  SBLAS_E_INVALID for
 * a bad op or nd. */
int sblas_krylov_scalar_step_ref(int op, int nd, int flag, const double *d, double *block, double rtol, double atol, int64_t max_iter);

/* The multi-column dot on its own: out[k * s + j] = (column j of x[k], column j of y[k]) for k < ndots <= 3, one pass
 * over memory and one fold; every result has the single pinned dot's bits.  x, y: HOST arrays of ndots device pointers
 * to n x s row-major blocks, ldx, ldy: HOST arrays of their leading dimensions (>= s); out: ndots * s doubles on the
 * device.  workspace: at least ..._dot_workspace(n, s, ndots) bytes on the device, 8-byte aligned (SBLAS_E_WORKSPACE when
 * missing or short); the first stage leaves dot k, column j, cell c at workspace[(k * s + j) * cells + c].  Operands need
 * 8-byte alignment only: a 16-byte-wide path is taken when every base and leading dimension allows it, with the same
 * bits.  Stream-ordered, allocates nothing, never synchronises, graph-capturable. */
size_t sblas_hip_krylov_multi_dot_workspace(int64_t n, int nrhs, int ndots);
int sblas_hip_krylov_multi_dot_f64(int dev, void *stream, int64_t n, int nrhs, int ndots, const double *const *x, const int64_t *ldx,
                                   const double *const *y, const int64_t *ldy, double *out, void *workspace, size_t workspace_bytes);
/* One fused multi-column update on its own (what the solver launches).  op and the order of v: SBLAS_KRYLOV_UP_*;
 * jacobi != 0 adds dinv (n entries, its ld is not read) and the preconditioned block at the single update's places.
 * scalars: s device blocks of 16 slots, block j at scalars + 16 j -- [0] status as int64 (anything but
 * SBLAS_KRYLOV_RUNNING: the call neither reads nor writes column j), [4] alpha, [5] beta, [6] omega.  v: a HOST array of
 * nv device pointers, ld: a HOST array of nv leading dimensions.  partial: device doubles, dot k of the pass, column j,
 * cell c at partial[(k * s + j) * cells + c] (NULL for an update without one). */
int sblas_hip_krylov_multi_update_f64(int dev, void *stream, int op, int jacobi, int64_t n, int nrhs, const double *scalars,
                                      double *const *v, const int64_t *ld, int nv, double *partial);

/* The plan.  create makes and owns an SpMM plan for width s on (rowptr, colidx), the SpMM's workspace, the work blocks
 * (leading dimension s), the partial sums and s scalar blocks; it may synchronise `stream`, and nothing after it
 * allocates.  The plan keeps the POINTERS rowptr and colidx, which must outlive it. */
int sblas_hip_krylov_multi_plan_create(int dev, void *stream, int method, int64_t n, int64_t nnz, const int32_t *rowptr,
                                       const int32_t *colidx, int nrhs, int precond, void **plan_out);
/* out: [0] n [1] nnz [2] method [3] precond [4] s [5] work blocks owned [6] bytes of one [7] bytes of the partials [8]
 * bytes of the scalar blocks [9] bytes of the SpMM's workspace [10] device bytes held (the SpMM plan's own apart) [11]
 * launches of one iteration without the products' (sblas_krylov_multi_launches with spmm_launches 0) */
int sblas_hip_krylov_multi_plan_info(const void *plan, int64_t out[12]);
int sblas_hip_krylov_multi_plan_destroy(void *plan);
/* start: per column |b_j|, r_j = b_j - A x_j (A X by the SpMM, then one rounded difference), the test at iteration 0 and
 * the first direction.  X on entry holds the initial guesses and is updated in place by iterate; it must not overlap B.
 * val, dinv (the inverse diagonal for JACOBI, ignored for NONE), B and X must stay valid and unchanged by others until
 * the solve is over.  ldb, ldx >= s; rtol, atol >= 0, max_iter >= 0, the same for every column.  Stream-ordered on the
 * calling thread's current device, which must be the plan's; allocates nothing, never synchronises.  start clears the
 * work blocks first: a column frozen from the start is never written but is still multiplied, so a solve's bits depend
 * on its own operands alone, not on what an earlier solve left in the plan.  X must not overlap B as address ranges
 * (two interleaved column slices of one wider tensor count as overlapping). */
int sblas_hip_krylov_multi_start(void *plan, void *stream, const double *val, const double *dinv, const double *B, int64_t ldb,
                                 double *X, int64_t ldx, double rtol, double atol, int64_t max_iter);
/* iterate: enqueues k lockstep iterations -- a fixed linear chain of launches, no allocation, no synchronisation
 * (graph-capturable).  SBLAS_E_INVALID before start. */
int sblas_hip_krylov_multi_iterate(void *plan, void *stream, int64_t k);
/* status: copies the scalar blocks back and synchronises `stream` -- the only call of a solve that does.  out: s x 8
 * doubles, column j's at out + 8 j in the order of sblas_hip_krylov_status. */
int sblas_hip_krylov_multi_status(const void *plan, void *stream, double *out);

#ifdef __cplusplus
}
#endif
#endif /* SBLAS_HIP_KRYLOV_MULTI_H */
