/* sblas_hip_amg_multi.h -- the AMG cycle on a block of columns, and its seat under the multi-right-hand-side Krylov
 * solvers.  Additive: sblas_hip.h includes this file, and every entry point declared there or in the
 * other headers keeps its signature and its bits; a plan that never calls sblas_hip_amg_plan_reserve_multi keeps its
 * bytes. */
#ifndef SBLAS_HIP_AMG_MULTI_H
#define SBLAS_HIP_AMG_MULTI_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * Z = M^-1 R for R, Z of n rows and s columns, ROW-MAJOR with a leading dimension >= s (the block convention of
 * sblas_hip_krylov_multi.h), 1 <= s <= SBLAS_AMG_MULTI_MAX_RHS: one V(nu, nu) cycle on all columns at once.
 *   - the contract: column j of Z has EXACTLY the bits sblas_hip_amg_plan_apply gives on column j of R, on the same plan
 *     after the same setup -- for every s, every leading dimension, every alignment, both prolongators and both
 *     aggregation modes.  Every kernel of the cycle is separable by column: a row's sum is taken per column in the pinned
 *     lane order (G(p) lanes by stored length, lane l the entries l, l + G, ... with one fused multiply-add each from
 *     +0, then the butterfly), the plain restriction adds an aggregate's members ascending from +0 per column, and
 *     everything else is rounded operation by operation.  No column of the cycle can reach another column: a NaN column
 *     gives its own column of NaN and nobody else's, a zero column gives a zero column.
 *   - a walk call is still ONE launch whatever s is: a block cycle has the launches sblas_amg_launches counts.  The row kernels
 *     run a grid of unit blocks x ceil(s / 8) workgroups, a lane holding eight columns of its entry's row (four
 *     16-byte loads when every base and leading dimension of the launch is a multiple of 16 bytes, else double by
 *     double: same values, same order, same bits).
 *   - the level vectors of a block cycle are the plan's (sblas_hip_amg_plan_reserve_multi), at leading dimension s.
 *     Padding columns j >= s of R and Z are never read or written.
 *   - the Chebyshev smoother (sblas_hip_amg_plan_setup_ex) has no block form: apply_multi refuses a plan whose last
 *     setup chose it.
 * ------------------------------------------------------------------------------------- */
#define SBLAS_AMG_MULTI_MAX_RHS 64
#define SBLAS_AMG_MULTI_TILE 8 /* columns of one workgroup of a row kernel */

/* HOST functions (no GPU call; testable alone).  limits: [0] the most columns [1] columns of a tile [2] threads of a
 * workgroup [3] reserved, 0. */
int sblas_amg_multi_limits(int64_t out[4]);
/* Workgroups of one multi-column row kernel over `units` four-lane units: [0] unit blocks = ceil(units / 64) [1] tiles =
 * ceil(s / 8) [2] their product, the grid [3] columns of the last tile.  SBLAS_E_INVALID for units < 0 or s outside
 * [1, 64]. */
int sblas_amg_multi_grid(int64_t units, int nrhs, int64_t out[4]);
/* SBLAS_OK when a multi-right-hand-side solver plan takes this preconditioner kind WITH a plan of that kind
 * (sblas_hip_krylov_multi_plan_create_ex): SBLAS_PRECOND_AMG alone.  ILU(0) is seated as a PAIR of solve plans through
 * a create of its own (sblas_hip_sptrsm_tile.h) and stays refused here; Chebyshev waits on a block polynomial of its own. */
int sblas_krylov_multi_precond_plan_ok(int precond);
/* Launches of ONE lockstep iteration with a product of spmm_launches launches and an applied preconditioner of
 * precond_launches launches.  NONE and JACOBI (precond_launches must be 0): sblas_krylov_multi_launches.  AMG: PCG
 * spmm + 5 + (precond_launches + 2) -- the cycle, the dots (r, z) and their fold; BiCGStab 2 spmm + 8 + 2
 * precond_launches.  -1 for a bad method, any other kind or a negative count. */
int64_t sblas_krylov_multi_launches_ex(int method, int precond, int64_t spmm_launches, int64_t precond_launches);

/* The block cycle's level vectors: for every level x0 | x1 | res | b of n_l x nrhs doubles.  Only grows: a request
 * at or below the reserved width changes nothing.  It allocates, so it may synchronise and is refused
 * (SBLAS_E_INVALID) while `stream` is capturing; it is the only call of this header that allocates. */
int sblas_hip_amg_plan_reserve_multi(void *plan, void *stream, int nrhs);
/* out: [0] the reserved width [1] the bytes reserved [2] launches of one block cycle (sblas_hip_amg_plan_info's [5]:
 * a walk call is one launch whatever s is) [3] reserved, 0 */
int sblas_hip_amg_plan_multi_info(const void *plan, int64_t out[4]);
/* Z = M^-1 R by one block cycle.  Stream-ordered on the calling thread's current device, which must be the plan's;
 * allocates nothing, never synchronises, graph-capturable.  SBLAS_E_INVALID for a plan that is not set up or whose
 * last setup chose the Chebyshev smoother, nrhs outside [1, 64], ldr or ldz below nrhs, a base that is not 8-byte
 * aligned, R overlapping Z as address ranges, or another device; SBLAS_E_WORKSPACE for nrhs above the reserved
 * width.  Every refusal comes before any launch. */
int sblas_hip_amg_plan_apply_multi(const void *plan, void *stream, int nrhs, const double *R, int64_t ldr, double *Z, int64_t ldz);

/* One launch of a block kernel on level `level` (what the block cycle launches), on the caller's blocks; the modes and
 * the refusals of sblas_hip_amg_sweep_f64 / _restrict_f64 / _prolong_f64, and those of apply_multi for the widths,
 * leading dimensions and alignment.  Y must overlap neither B nor X.  Restrict and prolong go by the plan's
 * prolongator: the aggregates' sums and the injection on a plain plan, rows of R and P on a smoothed one. */
int sblas_hip_amg_sweep_multi_f64(const void *plan, void *stream, int level, int mode, int nrhs, const double *B, int64_t ldb,
                                  const double *X, int64_t ldx, double *Y, int64_t ldy);
int sblas_hip_amg_restrict_multi_f64(const void *plan, void *stream, int level, int nrhs, const double *RES, int64_t ldr, double *BC,
                                     int64_t ldc);
int sblas_hip_amg_prolong_multi_f64(const void *plan, void *stream, int level, double scale, int nrhs, const double *E, int64_t lde,
                                    double *X, int64_t ldx);

/* sblas_hip_krylov_multi_plan_create with a preconditioner plan.  NONE / JACOBI with precond_plan NULL: the old
 * create.  SBLAS_PRECOND_AMG with an AMG plan made on this device for this very structure
 * (sblas_hip_amg_plan_speaks_for): the solver reserves the plan's level vectors for nrhs columns and applies the block
 * cycle where the single solver applies the cycle -- PCG on R into Z, BiCGStab on P into P^ and on S into S^.  Every
 * other kind, or a plan where none belongs, is SBLAS_E_INVALID.  The solver keeps the POINTER precond_plan, which must
 * outlive it; start takes no dinv and refuses a plan that is not set up or whose last setup chose the Chebyshev
 * smoother.  The freeze: the block cycle runs on ALL columns, into work blocks only, never into X; a frozen column's
 * operand no longer changes, so its result is recomputed to the same bits.  Two solvers seated on one AMG plan share
 * its level vectors, as two single solvers do: they must not run at the same time.  sblas_hip_krylov_multi_plan_info
 * then reads AMG in [3], and [11] counts through sblas_krylov_multi_launches_ex with the plan's cycle. */
int sblas_hip_krylov_multi_plan_create_ex(int dev, void *stream, int method, int64_t n, int64_t nnz, const int32_t *rowptr,
                                          const int32_t *colidx, int nrhs, int precond, void *precond_plan, void **plan_out);

#ifdef __cplusplus
}
#endif
#endif /* SBLAS_HIP_AMG_MULTI_H */
