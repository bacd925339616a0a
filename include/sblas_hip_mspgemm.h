/* sblas_hip_mspgemm.h -- masked SpGEMM: out = M o (X * Y^T), the product of two sparse matrices evaluated only on a given
 * CSR pattern, on a device plan that re-multiplies.  Additive: sblas_hip.h includes this file, and every
 * entry point declared there keeps its signature and its bits. */
#ifndef SBLAS_HIP_MSPGEMM_H
#define SBLAS_HIP_MSPGEMM_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * Masked SpGEMM, the "NT" form:  out = M o (X * Y^T)   X: m x k CSR, Y: n x k CSR, M: an m x n CSR pattern (no values);
 * fp64 values, int32 indices; every dimension and nnz below 2^31.  A plan: create checks and copies the three structures
 * once, numeric fills out (nnz(M) doubles, in M's stored order) for new values of X and Y.  Rows of all three may be
 * unsorted and hold duplicates, as everywhere else; empty rows, m, n, k = 0 and nnz = 0 are valid.  The contract, for every
 * stored mask entry t = (i, j), duplicates included (each duplicate gets the same value):
 *   (V) values: list the pairs (e, g), e a stored entry of X's row i and g a stored entry of Y's row j, with
 *       col_X(e) == col_Y(g); e is the major index and both run in stored order.  Each product is x_e * y_g with one
 *       rounding; out[t] is the first product with each later one added to it one at a time in that order,
 *       ((p1 + p2) + p3) + ..., plain fp64 adds; no product is contracted with an add; a single product is copied (-0.0
 *       stays -0.0); no pair gives +0.0.  Only matched pairs contribute: an Inf or NaN stored in X or Y at a column the
 *       other row does not hold never reaches out (a dense X Y^T followed by a mask would make a NaN of it).  (Which NaN
 *       a sum holds -- its sign and payload -- is the adder's choice where IEEE 754 leaves it open; that a NaN is there is
 *       part of the contract.);
 *   (I) independence: the bits of out[t] are a function of X's row i as stored and Y's row j as stored -- not of t's
 *       position, the internal path that took it, workgroup or chunk boundaries, or pointer alignment;
 *   (D) determinism: no floating-point atomics and nothing that depends on scheduling; the same inputs give the same bits
 *       on every run and under graph replay;
 *   (S) the plan's structure work never looks at values.
 * Why this order: it is SpGEMM's.  With (rowptr_c, colidx_c) the structure of C = A * B from the SpGEMM plan (A: m x k,
 * B: k x n) and (colptr, rowidx, valT) B's transpose from the transpose plan -- a column lists its entries by ascending
 * row, duplicates in stored order --, the masked product with M = C's pattern, X = A and Y = (colptr, rowidx, valT) lists,
 * for C[i, j], A's entries of row i in stored order and for each the entries (k, j) of B in stored order: SpGEMM's (V).
 * out then holds sblas_hip_spgemm_plan_numeric's bits exactly, for every input, unsorted rows and duplicates included.
 * Both gradients of C = A * B are of this form, with no transposed kernel: dA = A's pattern o (dC * B^T) pairs row i of
 * dC with row k of B; dB = B's pattern o (A^T * (dC^T)^T) pairs row k of A^T with row j of dC^T.
 * Two paths stand behind the contract; one pass over colidx_x and one over colidx_y at create decide between them for the
 * whole plan.  The sorted path takes the plan when every row of X and of Y is strictly ascending (sorted, no duplicates:
 * what coo_to_csr "sum", the COO plan, the SpGEMM and GEAM plans' csr() and the transpose plan's csc() of a duplicate-free
 * matrix produce).  Matches are then unique and ascending in the shared column.  It is parallel over mask entries, not
 * rows: a lane takes one entry, walks the shorter of the two rows and binary-searches the longer, O(min log max); the X
 * row a wave's first entry names is staged in LDS when it has at most sblas_mspgemm_limits()[0] entries.  The general path
 * takes every other plan, or every plan under SBLAS_MSPGEMM_GENERAL: a lane per mask entry walks X's row in stored order
 * and for each entry Y's row in stored order.  It is quadratic in the row lengths, correct for everything, and the slow
 * path; forced on sorted input it gives the sorted path's bits.
 * ------------------------------------------------------------------------------------- */
#define SBLAS_MSPGEMM_AUTO 0
#define SBLAS_MSPGEMM_GENERAL 1 /* the general path whatever the rows look like */
/* a plan's path, as sblas_hip_mspgemm_plan_info reports it */
#define SBLAS_MSPGEMM_PATH_SORTED 0
#define SBLAS_MSPGEMM_PATH_GENERAL 1

/* HOST functions (no GPU call; testable alone). */
/* out: [0] the longest X row (entries) a wave stages in LDS [1] lanes, hence mask entries, per workgroup [2], [3] 0 */
int sblas_mspgemm_limits(int64_t out[4]);
/* The contract as a scalar loop over HOST arrays: out (rowptr_m[m] doubles).  SBLAS_E_INVALID for a negative size, a
 * missing pointer, a rowptr that does not start at 0 or steps down, a mask column outside [0, n) or an X or Y column
 * outside [0, k); nothing is read through an index before it is known to be in range, and nothing is written then. */
int sblas_mspgemm_ref(int64_t m, int64_t n, int64_t k, const int32_t *rowptr_m, const int32_t *colidx_m,
                      const int32_t *rowptr_x, const int32_t *colidx_x, const double *val_x, const int32_t *rowptr_y,
                      const int32_t *colidx_y, const double *val_y, double *out);

/* create: checks on the device first that the three rowptr start at 0 and never step down and that every column index is
 * in range -- mask columns below n, X and Y columns below k -- (SBLAS_E_INVALID, nothing else is launched), decides the
 * path, and copies the three structures into the plan, which need not outlive create: numeric needs only values.  May
 * synchronise `stream` several times.  flags: SBLAS_MSPGEMM_AUTO or SBLAS_MSPGEMM_GENERAL. */
int sblas_hip_mspgemm_plan_create(int dev, void *stream, int64_t m, int64_t n, int64_t k, const int32_t *rowptr_m,
                                  const int32_t *colidx_m, const int32_t *rowptr_x, const int32_t *colidx_x,
                                  const int32_t *rowptr_y, const int32_t *colidx_y, int flags, void **plan_out);
/* out: [0] m [1] n [2] k [3] nnz(M) [4] nnz(X) [5] nnz(Y) [6] the path, SBLAS_MSPGEMM_PATH_* [7] X strictly ascending
 * (0/1) [8] Y strictly ascending (0/1) [9] launches of one numeric [10] bytes held [11] flags */
int sblas_hip_mspgemm_plan_info(const void *plan, int64_t out[12]);
/* out (nnz(M)) from val_x and val_y, in X's and Y's stored order.  Stream-ordered on the calling thread's current device;
 * allocates nothing, never synchronises, graph-capturable; one call at a time per plan.  out must not overlap val_x or
 * val_y.  SBLAS_E_INVALID for a missing pointer and when the current device is not the plan's. */
int sblas_hip_mspgemm_plan_numeric(const void *plan, void *stream, const double *val_x, const double *val_y, double *out);
int sblas_hip_mspgemm_plan_destroy(void *plan);

#ifdef __cplusplus
}
#endif
#endif /* SBLAS_HIP_MSPGEMM_H */
