/* sblas_hip_sddmm_narrow.h -- the narrow SDDMM: out[e] = alpha * <X[row(e), :k], Y[col(e), :k]> + beta * out[e] for k <= 8
 * on a part of a CSR pattern.  Additive: sblas_hip.h includes this file, and every entry point declared
 * there keeps its signature and its bits. */
#ifndef SBLAS_HIP_SDDMM_NARROW_H
#define SBLAS_HIP_SDDMM_NARROW_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * Narrow SDDMM.  The pattern is rows x cols CSR with int32 indices (rows may be unsorted and hold duplicates; empty rows,
 * rows = 0 and nnz = 0 are valid); X is rows x k at ldx >= k and Y is cols x k at ldy >= k, both row-major fp64; 1 <= k
 * <= 8; out holds one fp64 per stored entry.  The contract:
 *   (P) part: an entry e at (r, c) is inside SBLAS_PART_ALL always, SBLAS_PART_LOWER when c <= r, SBLAS_PART_UPPER when
 *       c >= r, SBLAS_PART_STRICT_LOWER when c < r and SBLAS_PART_STRICT_UPPER when c > r.  An entry outside the part
 *       gets +0.0 when beta == 0 and beta * out[e] (one rounding) otherwise; its rows of X and Y are never read, so an
 *       Inf or NaN there does not show;
 *   (V) values, for an entry inside the part: the order of sblas_hip_sddmm_csr_f64_i32 at the same k, of which this is
 *       the statement for k <= 8.  Pad both rows with +0 to kp elements, kp = 2 for k <= 2, 4 for k <= 4 and 8 beyond.
 *       k <= 4: s = +0, then s = fma(x_j, y_j, s) for j = 0 .. kp - 1.  5 <= k <= 8: s0 over j = 0, 1, 4, 5 and s1 over
 *       j = 2, 3, 6, 7, each from +0 by fma in that order, then s = s0 + s1.  (A padded step is fma(+0, +0, s): it
 *       leaves s alone, except that a sum that is -0 becomes +0.)  Then out[e] = alpha * s when beta == 0, which never
 *       reads out, and fma(beta, out[e], alpha * s) otherwise.  For SBLAS_PART_ALL the result equals
 *       sblas_hip_sddmm_csr_f64_i32 on row-major operands bit for bit;
 *   (I) independence: the bits of out[e] are a function of the two rows, alpha, beta and the old out[e] -- not of the
 *       entry's place, the workgroup that took it, the leading dimensions or any pointer's alignment;
 *   (D) determinism: one launch, no atomics on global memory, nothing that depends on scheduling.
 * ------------------------------------------------------------------------------------- */
#define SBLAS_PART_ALL 0
#define SBLAS_PART_LOWER 1        /* col <= row */
#define SBLAS_PART_UPPER 2        /* col >= row */
#define SBLAS_PART_STRICT_LOWER 3 /* col <  row */
#define SBLAS_PART_STRICT_UPPER 4 /* col >  row */

/* HOST functions (no GPU call; testable alone). */
/* out: [0] the widest k, 8 [1] stored entries one workgroup takes [2] threads of a workgroup [3] consecutive entries
 * one lane owns.  SBLAS_E_INVALID for NULL. */
int sblas_sddmm_narrow_limits(int64_t out[4]);
/* The contract as a scalar loop over HOST arrays, with the device entry's arguments and refusals (dev and stream are
 * ignored).  It also refuses, before it reads an operand, a rowptr that does not start at 0, steps down or does not end
 * at nnz, and a column outside [0, cols). */
int sblas_sddmm_narrow_ref(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr,
                           const int32_t *colidx, const double *X, int64_t ldx, const double *Y, int64_t ldy, int k,
                           double alpha, double beta, int part, double *out);

/* DEVICE.  Stream-ordered on device dev (dev < 0: the calling thread's current device); one launch, no workspace,
 * allocates nothing, never synchronises, graph-capturable.  colidx, X, Y and out are read 16 bytes at a time where base
 * and leading dimension allow and 4 or 8 bytes at a time otherwise, with the same bits.  out must not overlap X or Y.
 * SBLAS_E_INVALID for k outside 1..8, a leading dimension below k, an unknown part, a negative size, rows, cols or nnz
 * at or above 2^31, a missing pointer, and entries without a place (nnz > 0 with rows = 0 or cols = 0).  nnz = 0
 * returns SBLAS_OK and launches nothing. */
int sblas_hip_sddmm_narrow_f64_i32(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr,
                                   const int32_t *colidx, const double *X, int64_t ldx, const double *Y, int64_t ldy, int k,
                                   double alpha, double beta, int part, double *out);

#ifdef __cplusplus
}
#endif
#endif /* SBLAS_HIP_SDDMM_NARROW_H */
