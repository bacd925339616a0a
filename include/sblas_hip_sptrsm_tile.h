/* sblas_hip_sptrsm_tile.h -- the triangular solve on a block of columns with the single solve's bits, and ILU(0)'s seat
 * under the multi-right-hand-side Krylov solvers.  Additive: sblas_hip.h includes this file, and every
 * entry point declared there or in the other headers keeps its signature and its bits. */
#ifndef SBLAS_HIP_SPTRSM_TILE_H
#define SBLAS_HIP_SPTRSM_TILE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * T X = alpha B for B, X of n rows and nrhs columns, ROW-MAJOR with a leading dimension >= nrhs (the block convention of
 * sblas_hip_krylov_multi.h), on an ordinary solve plan of sblas_hip.h's triangular-solve section: no new plan data.
 *   - the contract, stronger than the older SpSM entry's: column j of X has EXACTLY the bits the single planned solve
 *     (SpSV, the _sptrsv_f64_i32_planned entry) gives on column j of B -- for every nrhs, every leading dimension, every
 *     alignment and every schedule mode.  The kernels are the single solve's with every lane widened by a tile of eight
 *     columns: the same G(p) lanes by stored length, lane l the entries l, l + G, ... in stored order, one fused
 *     multiply-add per selected entry and column from +0, the same butterfly, the same three roundings at the end.  An
 *     entry outside the triangle is skipped, never multiplied by zero: neither its value nor X at its column is loaded.
 *     No column can reach another column: a NaN column of B gives its own column of NaN and nobody else's.
 *   - a launch of the single solve is still ONE launch whatever nrhs is: a wide level runs (its unit blocks) x
 *     ceil(nrhs / 8) workgroups, a chain launch ceil(nrhs / 8) workgroups, each walking the whole run of levels for its
 *     own eight columns.  Nothing waits across workgroups and there are no atomics.
 *   - a lane moves its eight doubles as four 16-byte accesses when the tile is full and both bases and both leading
 *     dimensions are multiples of 16 bytes, else double by double: same values, same order, same bits.  Padding columns
 *     j >= nrhs are never read or written.
 *   - in place (X == B with ldx == ldb) is allowed; any other overlap is undefined.
 * ------------------------------------------------------------------------------------- */
#define SBLAS_SPTRSM_TILE 8 /* columns of one workgroup */

/* HOST functions (no GPU call; testable alone).  limits: [0] columns of a tile [1] threads of a wide workgroup [2]
 * threads of a chain workgroup [3] the most workgroups of one launch. */
int sblas_sptrsm_tile_limits(int64_t out[4]);
/* Workgroups of one wide launch over `units` four-lane units: [0] unit blocks = ceil(units / 64) [1] tiles =
 * ceil(nrhs / 8) [2] their product, the grid [3] columns of the last tile.  A chain launch is [1] workgroups.
 * SBLAS_E_INVALID for units < 0, nrhs < 1 or a grid above limits [3]. */
int sblas_sptrsm_tile_grid(int64_t units, int64_t nrhs, int64_t out[4]);
/* SBLAS_OK when a multi-right-hand-side solver plan takes this preconditioner kind WITH a pair of solve plans
 * (the _create_pair entry below): SBLAS_PRECOND_ILU0 alone. */
int sblas_krylov_multi_precond_pair_ok(int precond);
/* Launches of ONE lockstep iteration with a product of spmm_launches launches and a pair seated whose solves take
 * lower_launches and upper_launches launches ([5] of each plan's info): the count with an AMG plan seated, with the two
 * solves in the cycle's place.  PCG spmm + 5 + (lower + upper + 2), BiCGStab 2 spmm + 8 + 2 (lower + upper).  -1 for a
 * bad method, any kind but ILU(0) or a negative count. */
int64_t sblas_krylov_multi_launches_pair(int method, int precond, int64_t spmm_launches, int64_t lower_launches, int64_t upper_launches);

/* The tiled solve.  The checks and the no-ops of the older SpSM entry: rowptr / colidx must be the plan's and the
 * current device the plan's, nrhs >= 0, ldb and ldx >= nrhs (SBLAS_E_INVALID otherwise, before anything is launched);
 * n == 0 and nrhs == 0 succeed and launch nothing.  B and X need 8-byte alignment.  An nrhs whose widest launch would
 * pass limits [3] workgroups is refused.  Stream-ordered on the calling thread's current device, allocates nothing, never
 * synchronises: the single solve's sequence of launches (graph-capturable as a linear chain) that takes new val on
 * every call. */
int sblas_hip_sptrsm_tiled_f64_i32_planned(const void *plan, void *stream, const int32_t *rowptr, const int32_t *colidx,
                                           const double *val, int64_t nrhs, double alpha, const double *B, int64_t ldb,
                                           double *X, int64_t ldx);

/* A multi-right-hand-side solver plan with ILU(0) seated: lower_plan and upper_plan are the two solve plans that consume a
 * factor -- SBLAS_FILL_LOWER with SBLAS_DIAG_UNIT and SBLAS_FILL_UPPER with SBLAS_DIAG_NON_UNIT -- made on this device on
 * this very rowptr / colidx with this n and nnz; anything else, or a NULL plan, is SBLAS_E_INVALID.  The solver keeps the
 * POINTERS, which must outlive it.  It applies M^-1 where the single solver does -- PCG on R into Z, BiCGStab on P into P^
 * and on S into S^ -- as OUT = L^-1 IN by the tiled solve and then OUT = U^-1 OUT in place: no further work block.  The
 * multi start's dinv argument carries the factor lu for such a plan (nnz values, as the single solver's lu_or_dinv) and
 * is refused when NULL.  The freeze: the two solves run on ALL columns, into work blocks only, never into X; a frozen
 * column's operand no longer changes, so its result is recomputed to the same bits.  The plan's info reads
 * SBLAS_PRECOND_ILU0 in [3], and [11] counts both solves (the _launches_pair function with spmm_launches 0).  The older
 * creates keep refusing ILU(0). */
int sblas_hip_krylov_multi_plan_create_pair(int dev, void *stream, int method, int64_t n, int64_t nnz, const int32_t *rowptr,
                                            const int32_t *colidx, int nrhs, const void *lower_plan, const void *upper_plan,
                                            void **plan_out);

#ifdef __cplusplus
}
#endif
#endif /* SBLAS_HIP_SPTRSM_TILE_H */
