/* sblas_hip_geam.h -- CSR addition C = alpha * A + beta * B on a device plan that re-adds.  Additive:
 * sblas_hip.h includes this file, and every entry point declared there keeps its signature and its bits. */
#ifndef SBLAS_HIP_GEAM_H
#define SBLAS_HIP_GEAM_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * GEAM:  C = alpha * A + beta * B   A, B and C: rows x cols CSR; fp64 values, int32 indices; rows, cols, nnz(A), nnz(B)
 * and nnz(C) below 2^31.  A plan: create does the symbolic work once, numeric fills C's values for new values of A and
 * B and new alpha / beta on the same structures.  A and B may have unsorted rows and duplicate entries, as everywhere
 * else; empty rows, rows = 0, cols = 0 and either or both nnz = 0 are valid.  The contract:
 *   (S) structure: row i of C stores column j exactly when A or B stores (i, j).  Columns within a row are ascending and
 *       distinct.  The structure never depends on the values or on alpha / beta: alpha = 0 drops nothing, a sum that
 *       cancels stays as a stored zero, and so do NaN and Inf.  rowptr_C has rows + 1 int32 entries; if nnz(C) would
 *       reach 2^31, create returns SBLAS_E_INVALID and makes no plan;
 *   (V) values: list the terms of C's row i in this order: first A's entries of row i in stored order, each as alpha * a
 *       with one rounding; then B's entries of row i in stored order, each as beta * b with one rounding.  The value of
 *       C[i, j] is the first term that lands on j with each later term that lands on j added to it one at a time in
 *       that order, ((t1 + t2) + t3) + ..., plain fp64 adds; no product is contracted with an add; a single term is
 *       copied (-0.0 stays -0.0).  Put another way, C is sblas_hip_coo_to_csr_f64_i32 under SBLAS_COO_SUM of the
 *       triplets (i, j, alpha * a) of A followed by the triplets (i, j, beta * b) of B, in structure and in values.
 *       (Which NaN a sum holds -- its sign and payload -- is the adder's choice where IEEE 754 leaves it open; that a
 *       NaN is there is part of the contract.);
 *   (I) independence: the bits of C's row i are a function of A's row i and B's row i, as stored, of alpha and of beta
 *       -- not of the row's index, its neighbours, the internal path that took it, workgroup boundaries, or pointer
 *       alignment;
 *   (D) determinism: no floating-point atomics and nothing that depends on scheduling; the same inputs give the same
 *       bits on every run and under graph replay;
 *   (M) maps: dest_a[e] (nnz(A) int32) and dest_b[e] (nnz(B) int32) give the entry of C where each input entry lands;
 *       a run of duplicates shares one entry.  They are ordinary device arrays the plan owns: the gradient of C's
 *       values with respect to A's and B's is a gather over them.
 * Two paths stand behind the contract; one pass over both colidx at create decides between them for the whole plan.
 * The sorted path takes the plan when every row of A and of B is strictly ascending (sorted, no duplicates: what
 * coo_to_csr "sum", the COO plan, the transpose plan's csc() and the SpGEMM plan's csr() produce).  It is parallel over
 * entries, not rows: every entry finds its place by one binary search in the other operand's row and one exclusive scan
 * over B's entries, and numeric is one launch over C's entries.  The general path takes every other
 * plan, or every plan under SBLAS_GEAM_GENERAL: the plan owns a COO plan (SBLAS_COO_SUM) over A's triplets followed by
 * B's, numeric scales both value arrays into a buffer of the plan and assembles.  It needs nnz(A) + nnz(B) < 2^31.
 * ------------------------------------------------------------------------------------- */
#define SBLAS_GEAM_AUTO 0
#define SBLAS_GEAM_GENERAL 1 /* the general path whatever the rows look like */
/* As AUTO, but the sorted path's numeric is the two-launch ordered scatter: A's terms written through dest_a, then B's added
 * (or, where no A entry matched, written) through dest_b.  The same bits; kept as the measured alternative. */
#define SBLAS_GEAM_SCATTER 2
/* a plan's path, as sblas_hip_geam_plan_info reports it */
#define SBLAS_GEAM_PATH_SORTED 0
#define SBLAS_GEAM_PATH_GENERAL 1

/* HOST functions (no GPU call; testable alone). */
/* SBLAS_OK when nnz_c fits an int32 index (below 2^31), else SBLAS_E_INVALID: create's check on the counted nnz(C) */
int sblas_geam_check_nnz(int64_t nnz_c);
/* The contract as a scalar loop over HOST arrays: rowptr_c (rows + 1), *nnz_c and, each when not NULL, colidx_c and val_c
 * (the caller sizes them for nnz(A) + nnz(B) entries, or for the *nnz_c of a first call that passed them NULL), dest_a
 * (nnz(A)) and dest_b (nnz(B)).  val_a and val_b may be NULL when val_c is.  SBLAS_E_INVALID for a negative size, a
 * missing pointer, a rowptr that does not start at 0 or steps down, a column outside [0, cols), or an nnz(C) of 2^31 or
 * more; nothing is read through an index before it is known to be in range. */
int sblas_geam_ref(int64_t rows, int64_t cols, const int32_t *rowptr_a, const int32_t *colidx_a, const double *val_a,
                   const int32_t *rowptr_b, const int32_t *colidx_b, const double *val_b, double alpha, double beta,
                   int32_t *rowptr_c, int32_t *colidx_c, double *val_c, int32_t *dest_a, int32_t *dest_b, int64_t *nnz_c);

/* create: checks on the device first that both rowptr start at 0 and never step down and that every column index is in
 * range (SBLAS_E_INVALID, nothing else is launched), decides the path, and builds rowptr_C, colidx_C and the maps.  May
 * synchronise `stream` several times.  A's and B's structures are NOT copied and need not outlive create: numeric reads
 * neither.  flags: SBLAS_GEAM_AUTO, SBLAS_GEAM_GENERAL or SBLAS_GEAM_SCATTER.  The general path refuses nnz(A) + nnz(B) >= 2^31
 * (SBLAS_E_INVALID).  The plan owns C's structure, the maps and, by path, their inverse over C's entries (sorted) or
 * the COO plan and the buffer of scaled values (general). */
int sblas_hip_geam_plan_create(int dev, void *stream, int64_t rows, int64_t cols, const int32_t *rowptr_a,
                               const int32_t *colidx_a, const int32_t *rowptr_b, const int32_t *colidx_b, int flags,
                               void **plan_out);
/* out: [0] rows [1] cols [2] nnz(A) [3] nnz(B) [4] nnz(C) [5] matched entries, nnz(A) + nnz(B) - nnz(C) [6] the path,
 * SBLAS_GEAM_PATH_* [7] A strictly ascending (0/1) [8] B strictly ascending (0/1) [9] launches of one numeric
 * [10] bytes held (the COO plan's included) [11] flags */
int sblas_hip_geam_plan_info(const void *plan, int64_t out[12]);
/* C's structure (either output may be NULL): rowptr_c (rows + 1), colidx_c (nnz(C)); ordinary device arrays that live
 * until the plan is destroyed: the SpMV, SpMM, transpose, ILU(0), AMG and solver plans are built on them unchanged */
int sblas_hip_geam_plan_csr(const void *plan, const int32_t **rowptr_c, const int32_t **colidx_c);
/* the maps of (M) (either output may be NULL): dest_a (nnz(A)), dest_b (nnz(B)); they live until the plan is destroyed */
int sblas_hip_geam_plan_maps(const void *plan, const int32_t **dest_a, const int32_t **dest_b);
/* val_c (nnz(C)) from val_a and val_b, in A's and B's stored order, and alpha and beta.  Stream-ordered on the calling
 * thread's current device; allocates nothing, never synchronises, graph-capturable; one call at a time per plan.
 * val_c must not overlap val_a or val_b: a call whose three extents (nnz(C), nnz(A), nnz(B) doubles) show an overlap is
 * refused.  SBLAS_E_INVALID for that, for a missing pointer, and when the current device is not the plan's. */
int sblas_hip_geam_plan_numeric(const void *plan, void *stream, const double *val_a, const double *val_b, double alpha,
                                double beta, double *val_c);
int sblas_hip_geam_plan_destroy(void *plan);

#ifdef __cplusplus
}
#endif
#endif /* SBLAS_HIP_GEAM_H */
