/*
 * sblas_hip.h -- C ABI of libsblas_hip.so, the MI355X (gfx950) core of the S-BLAS CSR
 * SpMV / SpMM hot path.
 *
 * The reference (tartarughina/S-BLAS) has no FFI: its boundary for this path is the set of
 * cuSPARSE / NCCL / CUDA-runtime calls made by the header templates sblas_spmm_csr_v1/_v2 and
 * sblas_spmv_csr_v1.  Every entry point below replaces one of those call sites and takes the
 * same information the replaced call received (plain pointers and sizes, no C++ or torch
 * types).  The header-template layer in s-blas_amd/include/ (sblas.h, matrix.h, spmm.h, spmv.h)
 * forwards to these functions; INTEGRATION.md shows the binding a reference maintainer adds.
 * The sparse-times-sparse product (sblas_hip_spgemm_plan_*: C = A * B for two CSR matrices, symbolic once, numeric per
 * set of values) has no counterpart in the reference; it follows the plan idiom of the transpose and COO plans below and
 * takes over the COO contract's left-to-right sum word for word.
 *
 * Conventions
 *   - all array arguments of the *_hip_* compute functions are DEVICE pointers on device `dev`
 *     (dev < 0: use the calling thread's current device);
 *   - `stream` is a hipStream_t passed as void* (NULL = the device's null stream); nothing in the
 *     compute functions allocates, frees or synchronises, so they are graph-capturable;
 *   - CSR is base-0, int32 indices, fp64 values; `rowptr` is relative to the colidx/val pointers
 *     that are passed (so the re-based row-block slices of method 2 work as they are);
 *   - dense B / C are COLUMN-major with leading dimensions ldb / ldc (the only layout the
 *     reference's GPU paths accept: spmm.h:91-98, :171-178);
 *   - return value 0 = success, otherwise one of SBLAS_E_* (see sblas_hip_error_string).
 */
#ifndef SBLAS_HIP_H
#define SBLAS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBLAS_OK 0
#define SBLAS_E_INVALID 1   /* bad argument (null pointer, negative size, ld too small) */
#define SBLAS_E_HIP 2       /* a HIP runtime call or kernel launch failed              */
#define SBLAS_E_WORKSPACE 3 /* workspace missing or too small                          */
#define SBLAS_E_RCCL 4      /* RCCL unavailable or a collective failed                 */
#define SBLAS_E_IO 5        /* MatrixMarket file could not be read / parsed            */
#define SBLAS_E_NOGPU 6     /* no HIP device visible                                   */
#define SBLAS_E_INTERNAL 7  /* a device loop made no progress: a bug, reported, not spun on */

int sblas_hip_version(void);
const char *sblas_hip_error_string(int code);
/* Number of visible HIP devices (0 when none / no driver).  Never initialises a context. */
int sblas_hip_device_count(void);

/* ---------------------------------------------------------------------------------------
 * SpMM:  C = alpha * A * B + beta * C        A: rows x cols CSR, B: cols x n, C: rows x n
 * Replaces cusparseSpMM_bufferSize + cusparseSpMM (NON_TRANSPOSE, ALG_DEFAULT, col-major) at
 *   spmm.h:134-149  (method 1: full A, B/C column block of n_i columns, real alpha/beta)
 *   spmm.h:239-251  (method 2: re-based row block A_i, C = Ccopy + start_row, ldc = M, alpha=beta=1)
 * The workspace plays the role of cuSPARSE's externalBuffer (spmm.h:140-141, :245-246): it
 * holds the row-major staging copy of B that the kernels gather from.
 * ------------------------------------------------------------------------------------- */
size_t sblas_hip_spmm_csr_f64_i32_workspace(int64_t rows, int64_t cols, int64_t nnz, int64_t n);

int sblas_hip_spmm_csr_f64_i32(int dev, void *stream,
                               int64_t rows, int64_t cols, int64_t nnz,
                               const int32_t *rowptr, const int32_t *colidx, const double *val,
                               const double *B, int64_t ldb, int64_t n,
                               double alpha, double beta,
                               double *C, int64_t ldc,
                               void *workspace, size_t workspace_bytes);

/* The two stages of the call above, exposed so that a caller that multiplies the same B more
 * than once (method 2 keeps B resident) or wants per-stage timing can drive them itself:
 *   stage 1: Bt ((cols + 1) x ldbt row-major, zero padded, last row all zero) <- B (cols x n col-major)
 *   stage 2: the row-panel SpMM kernels reading Bt.
 * ldbt = sblas_hip_spmm_ldbt(n).  Bt must be a buffer of sblas_hip_spmm_csr_f64_i32_workspace(rows, cols, nnz, n)
 * bytes: stage 2 keeps its panel verdicts behind the staging copy.  (The split form does not chunk columns:
 * (cols + 1) * ldbt * 8 must stay below 4 GiB; the one-call form walks wider B in column chunks.) */
int64_t sblas_hip_spmm_ldbt(int64_t n);
int sblas_hip_dense_to_rowmajor_f64(int dev, void *stream, int64_t cols, int64_t n,
                                    const double *B, int64_t ldb, double *Bt, int64_t ldbt);
int sblas_hip_spmm_csr_rowmajorB_f64_i32(int dev, void *stream,
                                         int64_t rows, int64_t cols, int64_t nnz,
                                         const int32_t *rowptr, const int32_t *colidx,
                                         const double *val,
                                         const double *Bt, int64_t ldbt, int64_t n,
                                         double alpha, double beta, double *C, int64_t ldc);

/* A per-matrix plan -- the slot cusparseSpMM_bufferSize / the workspace step occupy in the reference (spmm.h:134-141).
 * The unplanned call classifies A's row panels on the device on EVERY call (which stage-2 kernel computes a panel, the
 * matrix-wide votes, a row block's column range) and then launches every stage-2 kernel; those that find nothing to do
 * leave at once.  A is usually multiplied many times: sblas_hip_spmm_plan_create runs that analysis once for one
 * structure (rowptr, colidx) and one width n, keeps the verdicts in a device buffer of its own and looks at them once
 * on the host (it synchronises `stream`); a planned call then stages B and launches ONLY the kernels that have panels.
 * Results are bit-identical to the unplanned call.  The plan refers to the structure arrays it was made from: the
 * caller recreates it when their contents change (values may change freely).  One call at a time per plan (the
 * staging pass keeps its "B holds a non-finite value" flag in the plan's buffer).  A planned call allocates nothing
 * and never synchronises (graph-capturable); create / destroy do. */
int sblas_hip_spmm_plan_create(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz,
                               const int32_t *rowptr, const int32_t *colidx, int64_t n, void **plan_out);
int sblas_hip_spmm_plan_destroy(void *plan);
/* out: [0] planned at all (0: empty matrix or a pinned kernel selection -- calls run unplanned), panels for the
 * LDS-tiled [1] / direct [2] / matrix-core [3] kernels, [4] which direct kernel at 128+ staged columns (0 row per wave,
 * 1 row merging, 2 four rows per wave), [5] only the
 * block's column range of B is staged, [6] staged width, [7] rows per panel */
int sblas_hip_spmm_plan_info(const void *plan, int64_t out[8]);
/* A split plan: a plan as above whose very long rows are summed by many workgroups instead of one.  The direct kernels
 * compute a row inside one workgroup, so a row of 10^5-10^6 entries keeps one CU busy while the rest of the chip waits.
 * sblas_hip_spmm_plan_create_split makes the plan above, copies rowptr and the panel verdicts to the host once, and
 * cuts every row of split_min+ entries in a panel the direct kernels own (sblas_spmm_split_classify below) into pieces
 * of at most `piece` entries (split_min / piece <= 0: SBLAS_SPMM_SPLIT_MIN / SBLAS_SPMM_SPLIT_PIECE).  A planned call
 * launches the direct kernels in a form that leaves those rows alone, then one workgroup per piece and column tile
 * (sums into a partial row in the plan's buffer) and a fold kernel that adds a row's partials in piece order.
 *   - create / destroy allocate and synchronise `stream`; a planned call allocates nothing, never synchronises and may
 *     be captured in a graph, whatever the orders of B and C and however n is cut into column chunks;
 *   - one call at a time per plan (the partial sums live in the plan's buffer);
 *   - results: every row that is not split is bit-identical to the plain plan's; a split row is summed in another order
 *     (pieces, then the pieces in order, no atomics), so its last bits can differ -- the same on every call;
 *   - not split: rows of panels the LDS-tiled, lane-group or matrix-core kernels own, every row when the row-merging
 *     kernel takes the direct panels, and every row of an inactive plan (info[0] = 0);
 *   - a plan without split rows is the plain plan: the same kernels, the same bits. */
int sblas_hip_spmm_plan_create_split(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz,
                                     const int32_t *rowptr, const int32_t *colidx, int64_t n, int64_t split_min,
                                     int64_t piece, void **plan_out);
/* out: [0] split rows, [1] pieces, [2] nonzeros in split rows, [3] bytes of the partial-sum buffer (pieces x staged
 * width x 8).  All zero for a plan made by sblas_hip_spmm_plan_create. */
int sblas_hip_spmm_plan_split_info(const void *plan, int64_t out[4]);
int sblas_hip_spmm_csr_f64_i32_planned(const void *plan, int dev, void *stream,
                                       int64_t rows, int64_t cols, int64_t nnz,
                                       const int32_t *rowptr, const int32_t *colidx, const double *val,
                                       const double *B, int64_t ldb, int64_t n, double alpha, double beta,
                                       double *C, int64_t ldc, void *workspace, size_t workspace_bytes);

/* Diagnostics (synchronises the current device): how many row panels of the SpMM launches since the last reset
 * took the LDS-windowed path [0], the direct path because they are too sparse over their column span [1], or were
 * windowed and then recomputed by the in-kernel fallback (rows not in ascending column order) [2], or the matrix-core
 * (MFMA) path [3]. */
int sblas_hip_debug_spmm_panel_stats(uint64_t out[4], int reset);
/* Opt-in check of the CONTENTS of a CSR structure on the device (synchronises `stream`): row pointers ascending from 0 to
 * nnz, column indices inside [0, cols).  SBLAS_OK / SBLAS_E_INVALID.  The compute entry points trust the contents (as
 * cuSPARSE does); SBLAS_VALIDATE=1 makes every SpMM / SpMV call run this check first (debugging). */
int sblas_hip_debug_validate_csr_i32(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz,
                                     const int32_t *rowptr, const int32_t *colidx);
/* The library reads its experiment switches (SBLAS_SPMM_VARIANT, SBLAS_SPMV_VARIANT, ...; none changes a result) from
 * the environment once, at the first launch.  A process that changes them afterwards (the test-suite does) calls this
 * to have them read again. */
int sblas_hip_debug_reload_env(void);
/* Diagnostics for per-kernel timing (bench.py's roofline object): while enabled, the SpMM launcher brackets the
 * dominant stage-2 kernel (the LDS-windowed one) with two HIP events
 * on the launch stream; ..._last_kernel_ms waits for the second event of the most recent launch on the current device
 * and returns the elapsed time.  Off by default: a timed region is not perturbed. */
int sblas_hip_debug_spmm_kernel_events(int enable);
int sblas_hip_debug_spmm_last_kernel_ms(float *ms);

/* ---------------------------------------------------------------------------------------
 * SpMV:  y = alpha * A * x + beta * y
 * Replaces cusparseSpMV_bufferSize + cusparseSpMV at spmv.h:94-106 (no workspace is needed).
 * ------------------------------------------------------------------------------------- */
int sblas_hip_spmv_csr_f64_i32(int dev, void *stream,
                               int64_t rows, int64_t cols, int64_t nnz,
                               const int32_t *rowptr, const int32_t *colidx, const double *val,
                               const double *x, double alpha, double beta, double *y);

/* A per-matrix SpMV plan (the slot of rocSPARSE's csrmv_analysis / cusparseSpMV_preprocess).  The unplanned call above
 * picks one kernel for the whole matrix from nnz / rows.  sblas_hip_spmv_plan_create copies rowptr to the host once,
 * cuts the rows into work items of one kernel block each (sblas_spmv_plan_classify below: per 256-row tile the kernel its
 * rows ask for; a row longer than SBLAS_SPMV_SPLIT_MIN cut into pieces of SBLAS_SPMV_SPLIT_PIECE nonzeros that run on as
 * many workgroups), finds each LDS-window item's column window on the device and keeps all of it in a device buffer of
 * its own; a planned call launches one kernel per non-empty class, in a fixed order, on `stream`.
 *   - create / destroy allocate and synchronise `stream`; a planned call allocates nothing and never synchronises
 *     (graph-capturable);
 *   - the plan covers one structure: the same rowptr / colidx arrays and their contents.  Values (val, x) may change
 *     freely; a call whose device, rows, cols, nnz or structure pointers differ from the plan's returns SBLAS_E_INVALID;
 *   - one call at a time per plan (split rows keep their partial sums in the plan's buffer);
 *   - results: a matrix whose tiles all ask for the kernel the unplanned call picks gives the unplanned call's bits.
 *     Split rows are summed in another order (pieces in CSR order, then folded in piece order: deterministic, never
 *     atomics), so their last bits can differ from the unplanned call's;
 *   - a plan whose items are all of one lanes-per-row / stream / segmented class and has no split rows runs the
 *     unplanned launch (its items are the unplanned kernel's blocks);
 *   - SBLAS_SPMV_VARIANT set when the plan is made, or an empty matrix: the plan is inactive (info[0] = 0) and planned
 *     calls run the unplanned launcher;
 *   - SBLAS_VALIDATE=1: plan_create checks the structure on the device first (SBLAS_E_INVALID, no plan). */
int sblas_hip_spmv_plan_create(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz,
                               const int32_t *rowptr, const int32_t *colidx, void **plan_out);
int sblas_hip_spmv_plan_destroy(void *plan);
/* out: [0] planned at all (0: calls run unplanned), work items of the lanes-per-row [1], stream with 4096 [2] / 6144 [3]
 * products of LDS, segmented [4] and LDS-window [5] kernels, [6] split rows, [7] pieces of the split rows */
int sblas_hip_spmv_plan_info(const void *plan, int64_t out[8]);
/* SBLAS_OK when the plan speaks for this device (< 0: the current one), these sizes and exactly these structure
 * pointers, SBLAS_E_INVALID otherwise: what a planned call checks, for a caller that keeps the plan inside a plan */
int sblas_hip_spmv_plan_speaks_for(const void *plan, int dev, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr,
                                   const int32_t *colidx);
int sblas_hip_spmv_csr_f64_i32_planned(const void *plan, int dev, void *stream,
                                       int64_t rows, int64_t cols, int64_t nnz,
                                       const int32_t *rowptr, const int32_t *colidx, const double *val,
                                       const double *x, double alpha, double beta, double *y);

/* ---------------------------------------------------------------------------------------
 * y = beta * y + alpha * x  (elementwise, n elements)
 * Replaces the denseVector_plusEqual_denseVector launches at matrix.h:613-625 and :714-726
 * (kernel.h:27-38).  Note the argument order mirrors the kernel: y is updated in place.
 * ------------------------------------------------------------------------------------- */
int sblas_hip_axpby_f64(int dev, void *stream, int64_t n,
                        double alpha, const double *x, double beta, double *y);

/* ---------------------------------------------------------------------------------------
 * Partial-result merge over the GPUs of one node (RCCL over xGMI).
 * Replaces ncclGetUniqueId / ncclCommInitRank / ncclAllReduce / ncclCommDestroy at
 *   spmm.h:179-181,189,260-262,279 and spmv.h:43-45,58,115-118,134.
 * One process drives n_gpu devices (the reference's process model); the communicator set is
 * created once and reused (sblas_hip_comm_get caches per device list).  RCCL is dlopen'ed on
 * first use so that the library loads on machines without it.
 * When several ranks are mapped onto ONE physical device (devs[] all equal; used to rehearse
 * the g-way paths on a single-GPU box) the sum is done by an on-device kernel instead.
 * ------------------------------------------------------------------------------------- */
int sblas_hip_comm_get(int n_gpu, const int *devs, void **comm_out);
void sblas_hip_comm_release_all(void);
/* In-place sum all-reduce of `count` doubles; bufs[r] / streams[r] belong to rank r.
 * Issues the collective for every rank (grouped) from the calling thread. */
int sblas_hip_allreduce_sum_f64(void *comm, double *const *bufs, void *const *streams,
                                int64_t count);

/* Method-2 / SpMV merge without the all-reduce (fast path for spmm.h:222-283 and spmv.h:60-138: the zero-filled
 * M x N `C_copy`, the ncclAllReduce over all of it and the axpby launch).  The partial results of the nnz row-block
 * partition (matrix.h:356-395) are disjoint except for the rows a block boundary cuts, so rank q computes only its
 * own rows into a PACKED buffer partial[q] (num_rows[q] x N, column-major, leading dimension num_rows[q];
 * start_row[q] = starting_row_gpu[q], num_rows[q] = get_gpu_row_ptr_num(q) - 1), every rank receives the other
 * ranks' packed blocks into gather[r] (room for the sum of all blocks; own block is not copied) over RCCL
 * send/recv -- half the xGMI bytes of the all-reduce, no redundant adds -- and one kernel per rank does
 *   C_r[i, j] = beta * C_r[i, j] + alpha * sum_{q : row i in block q} partial_q[i - start_row[q], j].
 * Ranks folded onto one device skip the copies.  Stream-ordered after each rank's producers; never synchronises. */
int sblas_hip_merge_rowblocks_f64(void *comm, int64_t M, int64_t N, const int64_t *start_row,
                                  const int64_t *num_rows, double *const *partial, double *const *gather,
                                  double alpha, double beta, double *const *C, int64_t ldc, void *const *streams);
/* The scatter + alpha/beta pass alone, for callers that moved the blocks themselves (torch.distributed, MPI ...):
 * src[q] are g packed blocks resident on `device`. */
int sblas_hip_merge_rowblocks_local_f64(int device, void *stream, int64_t M, int64_t N, int g,
                                        const int64_t *start_row, const int64_t *num_rows,
                                        const double *const *src, double alpha, double beta, double *C, int64_t ldc);

/* ---------------------------------------------------------------------------------------
 * The other value / index types of the reference's templates.  sblas_spmm_csr_v1/_v2 and sblas_spmv_csr_v1 are
 * templated over <IdxType, DataType> and hand cuSPARSE getCudaDataType<float|double>() and
 * getCusparseIndexType<int32_t|int64_t>() (utility.h:302-316; spmm.h:109-118, :196-213; spmv.h:64-77, :115-118).
 * The entry points below take the two types as tags and untyped pointers; <SBLAS_I32, SBLAS_F64> forwards to the
 * tuned *_f64_i32 functions above, the other three combinations run the plain kernels of typed_kernels.hip (same
 * semantics, sums in the value type in CSR order; not tuned).  alpha / beta are passed as doubles and converted.
 * One divergence: the reference's method-2 SpMM all-reduces with ncclDouble whatever DataType is (spmm.h:260-262);
 * here the merge runs in the value type (as the reference's SpMV does, spmv.h:115-118).
 * ------------------------------------------------------------------------------------- */
#define SBLAS_F64 0
#define SBLAS_F32 1
#define SBLAS_I32 0
#define SBLAS_I64 1
size_t sblas_hip_spmm_csr_workspace(int vtype, int itype, int64_t rows, int64_t cols, int64_t nnz, int64_t n);
int sblas_hip_spmm_csr(int dev, void *stream, int vtype, int itype, int64_t rows, int64_t cols, int64_t nnz,
                       const void *rowptr, const void *colidx, const void *val, const void *B, int64_t ldb, int64_t n,
                       double alpha, double beta, void *C, int64_t ldc, void *workspace, size_t workspace_bytes);
int sblas_hip_spmv_csr(int dev, void *stream, int vtype, int itype, int64_t rows, int64_t cols, int64_t nnz,
                       const void *rowptr, const void *colidx, const void *val, const void *x, double alpha,
                       double beta, void *y);
/* kernel.h:27-38 in either value type */
int sblas_hip_axpby(int dev, void *stream, int vtype, int64_t n, double alpha, const void *x, double beta, void *y);
int sblas_hip_allreduce_sum(void *comm, int vtype, void *const *bufs, void *const *streams, int64_t count);
int sblas_hip_merge_rowblocks(void *comm, int vtype, int64_t M, int64_t N, const int64_t *start_row,
                              const int64_t *num_rows, void *const *partial, void *const *gather, double alpha,
                              double beta, void *const *C, int64_t ldc, void *const *streams);

/* ---------------------------------------------------------------------------------------
 * Row-major dense operands.  The entry points above take B and C column-major; these take each of them in either
 * order (order_b and order_c are independent; the calls above are the (COL, COL) case of these):
 *   SBLAS_COL_MAJOR: B[k + j * ldb] (ldb >= cols), C[r + j * ldc] (ldc >= rows)
 *   SBLAS_ROW_MAJOR: B[k * ldb + j] (ldb >= n),    C[r * ldc + j] (ldc >= n)   -- the layout of a contiguous torch
 *                    tensor, cuSPARSE / rocSPARSE ORDER_ROW
 * B's order reaches only the staging copy (a row-major B is copied row by row, no transpose), C's only the write-back
 * of the stage-2 kernels.  The summation order is the same for every layout: the row-major result is the transpose of
 * the column-major one bit for bit.  The workspace size (sblas_hip_spmm_csr_workspace, ..._f64_i32_workspace) and an
 * SpMM plan (sblas_hip_spmm_plan_create) do not depend on either order: one of each serves all four combinations.
 * <SBLAS_I32, SBLAS_F64> runs the tuned kernels (column chunking of wide B, range staging, plans and SBLAS_VALIDATE=1
 * as in sblas_hip_spmm_csr_f64_i32), the other type pairs the typed kernels.  An order outside {0, 1}, a leading
 * dimension below its minimum or a missing pointer returns SBLAS_E_INVALID before anything touches the device.
 * ------------------------------------------------------------------------------------- */
#define SBLAS_COL_MAJOR 0
#define SBLAS_ROW_MAJOR 1
int sblas_hip_spmm_csr_ordered(int dev, void *stream, int vtype, int itype, int64_t rows, int64_t cols, int64_t nnz,
                               const void *rowptr, const void *colidx, const void *val,
                               const void *B, int64_t ldb, int order_b, int64_t n, double alpha, double beta,
                               void *C, int64_t ldc, int order_c, void *workspace, size_t workspace_bytes);
int sblas_hip_spmm_csr_ordered_f64_i32_planned(const void *plan, int dev, void *stream, int64_t rows, int64_t cols,
                                               int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                                               const double *val, const double *B, int64_t ldb, int order_b, int64_t n,
                                               double alpha, double beta, double *C, int64_t ldc, int order_c,
                                               void *workspace, size_t workspace_bytes);
/* sblas_hip_merge_rowblocks with C in either order.  SBLAS_ROW_MAJOR: C[r] is row-major (ldc >= N) and so is every
 * packed block: partial[q] is num_rows[q] x N at leading dimension N (contiguous, as in the column-major form), and so
 * is its region of gather[r]; the RCCL send / recv moves the same bytes as for column-major C. */
int sblas_hip_merge_rowblocks_ordered(void *comm, int vtype, int order, int64_t M, int64_t N, const int64_t *start_row,
                                      const int64_t *num_rows, void *const *partial, void *const *gather, double alpha,
                                      double beta, void *const *C, int64_t ldc, void *const *streams);

/* ---------------------------------------------------------------------------------------
 * Transposed products: y = alpha * A^T x + beta * y and C = alpha * A^T B + beta * C (cuSPARSE / rocSPARSE opA =
 * TRANSPOSE).  A^T stored as CSR is A stored as CSC: colptr (cols + 1), rowidx (nnz), valT (nnz).  Column c lists its
 * entries in CSR order (ascending row; duplicates keep their CSR order), the order of a stable sort of colidx, so every
 * transposed row is summed in one defined order: the transpose uses no floating-point atomics and repeated runs are
 * bit-identical.  With those arrays on the device, A^T x is sblas_hip_spmv_csr_f64_i32[_planned] on (colptr, rowidx,
 * valT) with rows := cols and cols := rows, and A^T B the same for the SpMM entry points; the plan below does exactly that.
 * ------------------------------------------------------------------------------------- */
/* Bytes of workspace sblas_hip_csr_transpose_f64_i32 needs (0 when it needs none: nnz == 0 or cols <= 1).  Depends on nnz
 * alone otherwise: 16 per nonzero for the sort's keys and payloads plus 1 KiB per 4096 nonzeros of digit counts. */
size_t sblas_hip_csr_transpose_workspace(int64_t rows, int64_t cols, int64_t nnz);
/* CSR (rows x cols) -> CSC on the device: colptr[cols + 1], rowidx[nnz], valT[nnz] and perm[nnz] (perm[i] = the CSR
 * position of CSC entry i, so valT[i] = val[perm[i]]).  val and valT may both be NULL (structure only); perm may be NULL.
 * nnz, rows and cols up to 2^31 - 1.  A stable LSD radix sort of the column indices, one 8-bit pass per byte of cols - 1
 * (none for cols == 1).  Allocates nothing, never synchronises, graph-capturable; trusts the CSR contents like the other
 * compute calls (SBLAS_VALIDATE=1 checks them first).  workspace: 16-byte aligned, sblas_hip_csr_transpose_workspace bytes. */
int sblas_hip_csr_transpose_f64_i32(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz,
                                    const int32_t *rowptr, const int32_t *colidx, const double *val,
                                    int32_t *colptr, int32_t *rowidx, double *valT, int32_t *perm,
                                    void *workspace, size_t workspace_bytes);
/* dst[i] = src[idx[i]], i < n: refreshes valT from new values of A through perm.  Graph-capturable. */
int sblas_hip_gather_f64(int dev, void *stream, int64_t n, const int32_t *idx, const double *src, double *dst);

/* A transpose plan: A^T as CSR in buffers the plan owns (colptr, rowidx, valT, perm: (cols + 1) * 4 + 16 * nnz bytes),
 * an SpMV plan over them and, for n > 0, an SpMM plan of width n (flags & SBLAS_TRANSPOSE_SPLIT: a split SpMM plan,
 * sblas_hip_spmm_plan_create_split with the default limits).  A long column of A is a long row of A^T; the SpMV plan's
 * split items and the split SpMM plan handle it.
 *   - create allocates and synchronises `stream`.  It always checks the CSR on the device first
 *     (sblas_hip_debug_validate_csr_i32): SBLAS_E_INVALID, no plan, and no transpose kernel runs on a bad structure.
 *     cols up to 2^31 - 65 (A^T's rows).  A matrix with no columns makes a plan that holds nothing on the device (every
 *     product is empty);
 *   - the plan holds its own copy of the values: new values of A reach it ONLY through ..._update_values (one gather
 *     launch; allocates nothing, graph-capturable).  Unlike the other plans, changing val in place is not seen;
 *   - the product calls allocate nothing, never synchronise and may be captured in a graph.  They run the planned SpMV /
 *     SpMM on the plan's arrays, so their bits are those of the planned calls on the same CSC arrays.  An SpMM of a
 *     width other than the plan's runs the unplanned tuned SpMM (sblas_hip_spmm_csr_ordered) on them;
 *   - A^T's shape sets the operands: x has rows entries and y cols; B is rows x n (SBLAS_COL_MAJOR ldb >= rows,
 *     SBLAS_ROW_MAJOR ldb >= n), C is cols x n (ldc >= cols, or >= n row-major).  The SpMM workspace is
 *     sblas_hip_spmm_csr_f64_i32_workspace(cols, rows, nnz, n) -- A^T's shape, rows and cols swapped;
 *   - a call on another device than the plan's returns SBLAS_E_INVALID;
 *   - one call at a time per plan, as for the plans above. */
#define SBLAS_TRANSPOSE_SPLIT 1
int sblas_hip_transpose_plan_create(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz,
                                    const int32_t *rowptr, const int32_t *colidx, const double *val,
                                    int64_t n, int flags, void **plan_out);
int sblas_hip_transpose_plan_update_values(void *plan, void *stream, const double *val);
/* out: [0] the plan holds CSC arrays on the device, [1] nnz, [2] bytes of those arrays, [3] an SpMM plan exists, [4] its
 * width, [5] split rows of the SpMV plan, [6] split rows of the SpMM plan (rows of A^T = columns of A), [7] 0 */
int sblas_hip_transpose_plan_info(const void *plan, int64_t out[8]);
/* the plan's device arrays (any output may be NULL); they live until the plan is destroyed */
int sblas_hip_transpose_plan_csc(const void *plan, const int32_t **colptr, const int32_t **rowidx, const double **valT);
int sblas_hip_transpose_plan_destroy(void *plan);
/* y (cols) = alpha * A^T x (x: rows) + beta * y */
int sblas_hip_spmv_csr_t_f64_i32_planned(const void *plan, int dev, void *stream, const double *x,
                                         double alpha, double beta, double *y);
/* C (cols x n) = alpha * A^T B (B: rows x n) + beta * C, either order of B and C */
int sblas_hip_spmm_csr_t_f64_i32_planned(const void *plan, int dev, void *stream, const double *B, int64_t ldb,
                                         int order_b, int64_t n, double alpha, double beta, double *C, int64_t ldc,
                                         int order_c, void *workspace, size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------
 * CSR from COO triplets on the device, with re-assembly.  Input: nnz triplets (coo_row[k], coo_col[k], coo_val[k]) in
 * any order, duplicates allowed; int32 indices, fp64 values; 0 <= row < rows, 0 <= col < cols; rows, cols and nnz below
 * 2^31.  The contract:
 *   - order: entries sorted by (row, col), equal (row, col) pairs in input order -- numpy.lexsort((coo_col, coo_row)),
 *     which is stable.  perm[i] = the input position of sorted position i;
 *   - SBLAS_COO_KEEP: every triplet becomes one CSR entry: colidx[i] = coo_col[perm[i]], val[i] = coo_val[perm[i]],
 *     rowptr[r] = the number of triplets with row < r, runptr[i] = i (nnz + 1 entries).  Duplicates as stored: the form
 *     every other entry point accepts;
 *   - SBLAS_COO_SUM: one CSR entry per distinct (row, col).  Its value is the run's first value with each later value of
 *     the run added to it one at a time in input order, ((v1 + v2) + v3) + ..., plain fp64 adds; a run of one is copied
 *     (-0.0 stays -0.0).  The structure never depends on the values: a sum that cancels to zero stays as a stored zero,
 *     and so do NaN and Inf.  runptr has csr_nnz + 1 entries: runptr[e] is the sorted position where entry e's run
 *     starts, runptr[csr_nnz] = nnz.  csr_nnz = rowptr[rows];
 *   - no floating-point atomics and nothing that depends on scheduling: the same input gives the same bits on every
 *     run and under graph replay.
 * One lane adds a whole run, which is what fixes the order; assembly runs are short.  A run of a million duplicates is
 * added by one lane and is slow (the run's values are still fetched by a whole workgroup); there is no second
 * summation order for it.
 * ------------------------------------------------------------------------------------- */
#define SBLAS_COO_KEEP 0
#define SBLAS_COO_SUM 1
/* Bytes of workspace sblas_hip_coo_to_csr_f64_i32 needs: 0 for nnz <= 0, otherwise 16 per triplet for the sort's keys and
 * payloads (reused by the structure passes), 1 KiB per 4096 triplets of digit counts and the scans' block sums.  Depends
 * on nnz alone. */
size_t sblas_hip_coo_to_csr_workspace(int64_t rows, int64_t cols, int64_t nnz);
/* COO -> CSR on the device, one shot: rowptr[rows + 1], colidx, val and, when not NULL, perm[nnz] and runptr.  The caller
 * sizes colidx and val for nnz entries and runptr for nnz + 1; with SBLAS_COO_SUM the entry count is rowptr[rows] and
 * what lies beyond it (beyond runptr[count]) is unspecified.  coo_val and val are both given or both NULL (structure
 * only).  A stable LSD radix sort, 8 bits a pass: ceil(bits(cols - 1) / 8) + ceil(bits(rows - 1) / 8) passes (none for a
 * dimension of 1).  Stream-ordered, allocates nothing, never synchronises, graph-capturable; trusts the triplets like
 * the other compute calls -- except under SBLAS_VALIDATE=1, which checks the index ranges first and waits for the answer
 * (SBLAS_E_INVALID, nothing else runs).  nnz == 0, rows == 0 and cols == 0 are valid when no triplet needs a place.
 * workspace: 16-byte aligned, sblas_hip_coo_to_csr_workspace bytes. */
int sblas_hip_coo_to_csr_f64_i32(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz,
                                 const int32_t *coo_row, const int32_t *coo_col, const double *coo_val, int dup,
                                 int32_t *rowptr, int32_t *colidx, double *val, int32_t *perm, int32_t *runptr,
                                 void *workspace, size_t workspace_bytes);
/* An assembly plan: the structure is fixed, the values change (a time step, a Newton iteration).
 *   - create always checks the index ranges on the device first: a triplet outside the matrix returns SBLAS_E_INVALID, no
 *     plan is made and no sort kernel runs on it.  It then sorts once into buffers the plan owns (rowptr, colidx, perm,
 *     runptr: (rows + 1) * 4 + 12 * (nnz + 1) bytes), frees the sort workspace and synchronises `stream`;
 *   - rowptr and colidx are ordinary device arrays: the SpMV, SpMM and transpose plans are built on them unchanged;
 *   - assemble writes the CSR values of new triplet values: val_out[e] = the left-to-right sum of coo_val[perm[k]],
 *     k in [runptr[e], runptr[e + 1]) (SBLAS_COO_KEEP: the plain gather).  One launch on the calling thread's current
 *     device; allocates nothing, never synchronises, graph-capturable.  SBLAS_E_INVALID when the current device is not
 *     the plan's;
 *   - one call at a time per plan, as for the plans above. */
int sblas_hip_coo_plan_create(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz, const int32_t *coo_row,
                              const int32_t *coo_col, int dup, void **plan_out);
/* out: [0] rows, [1] cols, [2] input nnz, [3] CSR nnz, [4] longest run, [5] sort passes, [6] bytes held, [7] dup */
int sblas_hip_coo_plan_info(const void *plan, int64_t out[8]);
/* the plan's device arrays (any output may be NULL): rowptr (rows + 1), colidx (CSR nnz), perm (nnz), runptr (CSR nnz +
 * 1); they live until the plan is destroyed */
int sblas_hip_coo_plan_csr(const void *plan, const int32_t **rowptr, const int32_t **colidx, const int32_t **perm,
                           const int32_t **runptr);
int sblas_hip_coo_plan_assemble(const void *plan, void *stream, const double *coo_val, double *val_out);
int sblas_hip_coo_plan_destroy(void *plan);

/* ---------------------------------------------------------------------------------------
 * SpGEMM:  C = A * B   A: m x k CSR, B: k x n CSR, C: m x n CSR; fp64 values, int32 indices; m, k, n and every nnz
 * below 2^31.  A plan: create does the symbolic work once, numeric fills C's values for new values of A and B on the
 * same structure.  A and B may have unsorted rows and duplicate entries, as everywhere else; empty rows, m = 0, k = 0,
 * n = 0 and nnz = 0 are valid.  The contract:
 *   (S) structure: row i of C stores column j exactly when some stored a_ik and some stored b_kj exist.  Columns within
 *       a row are ascending and distinct.  The structure never depends on the values: a sum that cancels stays as a
 *       stored zero, and so do NaN and Inf.  rowptr_C has m + 1 int32 entries; if nnz(C) would reach 2^31, create
 *       returns SBLAS_E_INVALID and makes no plan;
 *   (V) values: number the products of C's row i by (position e of a_ik within A's row i, position f of b_kj within
 *       B's row k), e the major index, both in stored order.  Each product is a * b with one rounding.  The value of
 *       C[i, j] is the first product that lands on j with each later product that lands on j added to it one at a time
 *       in that numbering, ((p1 + p2) + p3) + ..., plain fp64 adds; a single product is copied (-0.0 stays -0.0).  Put
 *       another way, C is sblas_hip_coo_to_csr_f64_i32(..., SBLAS_COO_SUM) of the expanded triplets (i, j, a * b)
 *       listed in that numbering, in structure and in values.  (Which NaN a sum holds -- its sign and payload -- is
 *       the adder's choice where IEEE 754 leaves it open; that a NaN is there is part of the contract.);
 *   (I) independence: the bits of C's row i are a function of A's row i, as stored, and of the rows of B it names, as
 *       stored -- not of the row's index, its neighbours, the internal path that took it, chunk or workgroup
 *       boundaries, or pointer alignment;
 *   (D) determinism: no floating-point atomics and nothing that depends on scheduling; the same inputs give the same
 *       bits on every run and under graph replay.  (Integer LDS atomics set bitmap bits; no output bit depends on
 *       which lane comes first.)
 * Two paths stand behind the contract.  The row path takes a row of C when every row of B is strictly ascending (sorted,
 * no duplicates: what coo_to_csr "sum", the COO plan and the transpose plan's csc() produce; one pass over colidx_b at
 * create decides it) and the row's column span -- from the least first to the greatest last column of the B rows it
 * names -- is at most S_max: a wave, or a 16-lane group of it, owns the row and walks A's entries in stored order.  The
 * general path takes every other row: chunks of consecutive general rows are expanded into triplets, sorted and
 * run-summed by the COO passes.  sblas_hip_spgemm_classify is the host rule that decides (no GPU call; testable alone).
 * ------------------------------------------------------------------------------------- */
#define SBLAS_SPGEMM_AUTO 0
#define SBLAS_SPGEMM_GENERAL 1 /* every row through the general path */
/* a row's path, as sblas_hip_spgemm_classify reports it */
#define SBLAS_SPGEMM_PATH_EMPTY 0   /* no product: nothing runs, the C row is empty */
#define SBLAS_SPGEMM_PATH_ROW 1
#define SBLAS_SPGEMM_PATH_GENERAL 2
/* out: [0] S_max (columns), [1] LDS accumulator entries of the 64-lane form (a longer C row accumulates in val_c),
 * [2] default chunk cap (products), [3] 0 */
int sblas_hip_spgemm_limits(int64_t out[4]);
/* The host rule.  products[i]: the products of row i (int64: a total may pass 2^31); span[i]: its column span;
 * b_ascending: the verdict on B's rows; chunk_cap: 0 = default.  path[i] = SBLAS_SPGEMM_PATH_*: EMPTY when the row has
 * no product, else ROW when b_ascending, flags == SBLAS_SPGEMM_AUTO and span[i] <= S_max, else GENERAL.  The general
 * rows, numbered 0, 1, ... in row order, are cut into *n_chunks chunks: chunk c holds the general rows chunk_first[c] ..
 * chunk_first[c + 1] - 1 (n_chunks + 1 entries are written, at most m + 1), consecutive, each with at most chunk_cap
 * products unless it is a single row. */
int sblas_hip_spgemm_classify(int64_t m, const int64_t *products, const int64_t *span, int b_ascending, int flags,
                              int64_t chunk_cap, uint8_t *path /* m */, int64_t *chunk_first /* up to m + 1 */,
                              int64_t *n_chunks);
/* lanes that own a row-path row of a_len stored A entries: 16 while products <= 16 * a_len (the named B rows are short
 * on average) and span <= S_max / 4, else 64.  The order within the row is the same in both. */
int sblas_hip_spgemm_group_width(int64_t products, int64_t a_len, int64_t span);
/* SBLAS_OK when nnz_c fits an int32 index (below 2^31), else SBLAS_E_INVALID: create's check on the counted nnz(C) */
int sblas_hip_spgemm_check_nnz(int64_t nnz_c);
/* create: checks on the device first that both rowptr start at 0 and never step down and that every column index is in
 * range (SBLAS_E_INVALID, nothing else is launched), copies both structures into the plan, counts products and spans
 * in one pass over A's rows, applies the host rule, and builds rowptr_C and colidx_C.  Synchronises `stream` several
 * times.  A general row of more than 2^31 - 1 products is refused (SBLAS_E_INVALID).  The plan owns C's structure, the
 * copies of A's and B's, the row lists and the general path's workspace, which is sized by the largest chunk. */
int sblas_hip_spgemm_plan_create(int dev, void *stream, int64_t m, int64_t k, int64_t n, const int32_t *rowptr_a,
                                 const int32_t *colidx_a, const int32_t *rowptr_b, const int32_t *colidx_b, int flags,
                                 int64_t chunk_cap /* 0 = default */, void **plan_out);
/* out: [0] m [1] k [2] n [3] nnz(C) [4] products in total [5] rows on the row path [6] rows on the general path
 * [7] chunks [8] most products in one row [9] B strictly ascending (0/1) [10] bytes held [11] flags */
int sblas_hip_spgemm_plan_info(const void *plan, int64_t out[12]);
/* C's structure (either output may be NULL): rowptr_c (m + 1), colidx_c (nnz(C)); ordinary device arrays that live until
 * the plan is destroyed: the SpMV, SpMM and transpose plans are built on them unchanged */
int sblas_hip_spgemm_plan_csr(const void *plan, const int32_t **rowptr_c, const int32_t **colidx_c);
/* val_c (nnz(C)) from val_a and val_b, in A's and B's stored order.  Stream-ordered on the calling thread's current
 * device; allocates nothing, never synchronises, graph-capturable; one call at a time per plan.  The general path
 * sorts its chunks again on every call.  SBLAS_E_INVALID when the current device is not the plan's. */
int sblas_hip_spgemm_plan_numeric(const void *plan, void *stream, const double *val_a, const double *val_b, double *val_c);
int sblas_hip_spgemm_plan_destroy(void *plan);

/* ---------------------------------------------------------------------------------------
 * Sparse triangular solves on a level-scheduled plan:  T x = alpha * b  (SpSV)  and  T X = alpha * B  for nrhs
 * right-hand sides (SpSM); B and X row-major n x nrhs with leading dimensions ldb, ldx >= nrhs.
 *   - T is the lower or upper triangle (fill) of a square n x n CSR matrix, fp64 values, int32 indices, n and nnz below
 *     2^31.  Rows may be unsorted; off-diagonal duplicates add.  STORED ENTRIES IN THE OTHER TRIANGLE ARE IGNORED: a full
 *     matrix can be passed for a Gauss-Seidel sweep, and a combined ILU(0) factor (unit-lower L and upper U in one CSR)
 *     is solved by two plans on the same arrays.
 *   - SBLAS_DIAG_UNIT ignores stored diagonal entries and uses 1.  SBLAS_DIAG_NON_UNIT needs exactly one stored diagonal
 *     entry in every row: a missing or duplicated one, a column outside [0, n), a rowptr that does not start at 0, steps
 *     down or does not end at nnz make create fail with SBLAS_E_INVALID and report the first such row in *bad_row; no
 *     kernel runs on such a structure.  A numerically zero pivot is NOT checked: the division follows IEEE 754, and
 *     Inf / NaN spread to the rows that depend on it.
 *   - level(i) = 0 when row i has no selected off-diagonal entry (column < i for LOWER, > i for UPPER), else 1 + the
 *     greatest level of the rows they name.  The rows of one level are independent.  Two kernels: WIDE, one launch for
 *     one level; CHAIN, one launch of a single workgroup for a run of consecutive levels with a workgroup barrier
 *     between them.  Nothing waits across workgroups (no flag polling, no cooperative launch, no grid barrier), there
 *     are no atomics, and every loop's trip count comes from the plan.
 *   - results contract.  SpSV: the bits of x[i] are a function of row i's stored entries (columns and values, in stored
 *     order), the x values they name, b[i] and alpha -- NOT of the level structure, of the kernel that took the row, of
 *     the mode or of chain_rows.  A row of p stored entries (both triangles and the diagonal counted) belongs to
 *     G(p) = 4 (p <= 4), 16 (p <= 32) or 64 lanes; lane l sums the selected entries among the stored entries l, l + G,
 *     l + 2G, ... in that order, one fused multiply-add each from +0; the lanes fold by a butterfly (l ^ 1, l ^ 2, ...);
 *     then x[i] = (alpha * b[i] - sum) / t_ii with each of the three operations rounded on its own (t_ii = 1 under UNIT).
 *     SpSM: lanes run along the right-hand sides, and column j sums row i's selected entries one after another in
 *     stored order (fused multiply-adds from +0), then the same last expression: column j's bits are a function of
 *     column j of B alone, independent of nrhs, ldb and ldx.  They need not equal SpSV's.
 *   - in place (x == b; X == B with ldx == ldb) is allowed: row i alone reads b[i], and does so before it writes x[i].
 *     Partial overlap is undefined.
 *   - the transposed solve T^T x = alpha * b needs no kernel of its own: the transpose plan's csc() arrays are T^T as
 *     CSR arrays of the opposite fill, and a solve plan on them is the transposed solve.
 * ------------------------------------------------------------------------------------- */
#define SBLAS_FILL_LOWER 0
#define SBLAS_FILL_UPPER 1
#define SBLAS_DIAG_NON_UNIT 0
#define SBLAS_DIAG_UNIT 1
#define SBLAS_SPTRSV_AUTO 0       /* a level above chain_rows rows: one wide launch; a run of narrower levels: one chain launch */
#define SBLAS_SPTRSV_PER_LEVEL 1  /* every level a wide launch */
#define SBLAS_SPTRSV_CHAIN_ONLY 2 /* one chain launch for everything (tests: the chain kernel loops over a wide level) */
/* a launch's kind, as the schedule reports it */
#define SBLAS_SPTRSV_LAUNCH_WIDE 0
#define SBLAS_SPTRSV_LAUNCH_CHAIN 1
/* out: [0] default chain_rows, [1] threads of the chain workgroup, [2] longest row of 4 lanes, [3] longest row of 16 lanes */
int sblas_hip_sptrsv_limits(int64_t out[4]);
/* The host rule, on HOST arrays (no GPU call; testable alone).  Checks the structure as described above, in this order:
 * rowptr (*bad_row = the first row that ends before it starts; 0 when rowptr[0] != 0), then row by row the columns and,
 * under NON_UNIT, the diagonal.  level_out[i] = level(i); *n_levels = the greatest level + 1 (0 when n == 0).  bad_row may
 * be NULL; it is -1 on success. */
int sblas_sptrsv_levels(int64_t n, const int32_t *rowptr, const int32_t *colidx, int fill, int diag,
                        int32_t *level_out /* n */, int64_t *n_levels, int64_t *bad_row);
/* The launches of a solve over levels of widths[l] rows: launch q covers the levels launch_first_out[q] ..
 * launch_first_out[q + 1] - 1 (n_launches + 1 entries are written, at most n_levels + 1) and is of kind kind_out[q]
 * (SBLAS_SPTRSV_LAUNCH_*; a wide launch is always one level).  flags = SBLAS_SPTRSV_*; chain_rows: 0 = default. */
int sblas_sptrsv_schedule(int64_t n_levels, const int64_t *widths, int flags, int64_t chain_rows,
                          uint8_t *kind_out /* up to n_levels */, int64_t *launch_first_out /* up to n_levels + 1 */,
                          int64_t *n_launches);
/* The lanes of a level plan, on HOST arrays (no GPU call; testable alone): what the solves' and ILU(0)'s creates upload,
 * with the neutral record (row, unit number within the row) in place of theirs.  level[i] in [0, n_levels) is row i's
 * level; only the differences of rowptr are read.  perm_out: the rows by (level, row); level l is perm_out[level_ptr_out[l]
 * .. level_ptr_out[l + 1] - 1] and the units level_unit_ptr_out[l] .. level_unit_ptr_out[l + 1] - 1.  A unit is four lanes.
 * A row of p stored entries owns G(p) / 4 consecutive units, numbered unit_q_out = 0 .. G(p) / 4 - 1, and its first unit
 * lies a multiple of G(p) / 4 units from the start of its level; rows ascend inside a level; a unit that pads the
 * alignment has unit_row_out = -1 and unit_q_out = 0.  *n_units = the units of all levels.  Every output array may be
 * NULL: a call with all of them NULL sizes the unit arrays.  A level outside [0, n_levels) is SBLAS_E_INVALID. */
int sblas_sptrsv_pack(int64_t n, const int32_t *rowptr, const int32_t *level, int64_t n_levels, int32_t *perm_out /* n */,
                      int32_t *level_ptr_out /* n_levels + 1 */, int64_t *level_unit_ptr_out /* n_levels + 1 */,
                      int32_t *unit_row_out /* *n_units */, int32_t *unit_q_out /* *n_units */, int64_t *n_units);
/* create: copies rowptr and colidx to the host once, runs the host rule, and uploads the rows ordered by (level, row)
 * with each row's extent and diagonal position, the level pointer, and every level's rows packed into four-lane units
 * (a row of G lanes is G / 4 of them).  Synchronises `stream`.
 * The plan keeps the caller's rowptr / colidx POINTERS, which must outlive the plan and stay unchanged.  bad_row may be
 * NULL.  n == 0 succeeds. */
int sblas_hip_sptrsv_plan_create(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr,
                                 const int32_t *colidx, int fill, int diag, int flags, int64_t chain_rows /* 0 = default */,
                                 void **plan_out, int64_t *bad_row);
/* out: [0] n [1] nnz [2] fill [3] diag [4] levels [5] launches [6] wide launches [7] chain launches [8] rows of the widest
 * level [9] stored entries of the longest row [10] device bytes held [11] flags */
int sblas_hip_sptrsv_plan_info(const void *plan, int64_t out[12]);
/* SBLAS_OK when the plan lives on device `dev` (< 0: the current one) and was made for exactly these rowptr / colidx
 * pointers, SBLAS_E_INVALID otherwise: what a planned solve checks, for a caller that keeps the plan inside a plan */
int sblas_hip_sptrsv_plan_speaks_for(const void *plan, int dev, const int32_t *rowptr, const int32_t *colidx);
/* device views that live until the plan is destroyed (either output may be NULL; both NULL when n == 0): perm (n): the
 * rows by (level, row); level_ptr (levels + 1): level l is perm[level_ptr[l] .. level_ptr[l + 1] - 1] */
int sblas_hip_sptrsv_plan_order(const void *plan, const int32_t **perm, const int32_t **level_ptr);
int sblas_hip_sptrsv_plan_destroy(void *plan);
/* The solves.  Stream-ordered on the calling thread's current device; they allocate nothing and never synchronise: a
 * fixed sequence of launches (graph-capturable as a linear chain of nodes) that takes new `val` on every call.
 * rowptr / colidx must be the pointers the plan was made with, and the current device the plan's: SBLAS_E_INVALID
 * otherwise, before anything is launched.  n == 0 and nrhs == 0 succeed and launch nothing. */
int sblas_hip_sptrsv_f64_i32_planned(const void *plan, void *stream, const int32_t *rowptr, const int32_t *colidx,
                                     const double *val, double alpha, const double *b, double *x);
int sblas_hip_sptrsm_f64_i32_planned(const void *plan, void *stream, const int32_t *rowptr, const int32_t *colidx,
                                     const double *val, int64_t nrhs, double alpha, const double *B, int64_t ldb,
                                     double *X, int64_t ldx);

/* ---------------------------------------------------------------------------------------
 * ILU(0) on a level-scheduled plan, factored on the device:  lu = ILU0(A)  for a square n x n CSR matrix, fp64 values,
 * int32 indices, n and nnz below 2^31, with the same pattern in and out.  lu holds the strictly-lower entries of the
 * unit-lower L (its diagonal is not stored) and the diagonal and upper entries of U: exactly what two solve plans
 * (SBLAS_FILL_LOWER with SBLAS_DIAG_UNIT, and SBLAS_FILL_UPPER) on (rowptr, colidx, lu) consume.
 *   - structure.  Every row must be strictly ascending in column (sorted, nothing doubled: ILU(0) of a pattern with a
 *     doubled entry is not defined) and must store its diagonal.  create refuses anything else with SBLAS_E_INVALID,
 *     names the first bad row in *bad_row and launches nothing.  The checks run in this order: rowptr (as
 *     sblas_sptrsv_levels: starts at 0, never steps down; in create also: ends at nnz, reported as row n - 1, first of
 *     all), then every column's range in every row, then row by row the ascending order and the diagonal.
 *   - arithmetic: the row-wise (IKJ) elimination, and the bits are pinned.  w starts as row i of val and ends as row i of
 *     lu.  For the stored entries e of row i with column k < i, in stored (ascending) order: l = w[e] / lu[diag(k)],
 *     w[e] = l, and for every stored entry f of row k with column j > k, if row i stores column j at p:
 *     w[p] = w[p] - l * lu[f], the product rounded and then the difference rounded (no fused multiply-add).  No sum is
 *     ever folded across lanes: each entry receives its updates one after another in ascending k.  So the bits of lu are
 *     a function of val and the pattern alone -- NOT of the schedule, the mode, chain_rows, or of which lanes or kernel
 *     took a row -- and a ten-line scalar loop on the host reproduces them exactly.
 *   - pivots.  A zero pivot is NOT checked: the division follows IEEE 754, and Inf / NaN reach the dependants only.  The
 *     plan exposes each row's diagonal position as a device array (plan_diag): one gather inspects the pivots.
 *   - in place (lu == val) is allowed.  Partial overlap is undefined.
 *   - schedule: the lower solve's.  Row i needs the finished rows k < i it stores an entry for, so the levels are
 *     sblas_sptrsv_levels(LOWER, NON_UNIT) and the launches sblas_sptrsv_schedule: WIDE, one launch for one level; CHAIN,
 *     one launch of a single workgroup for a run of consecutive levels with a workgroup barrier between them.  Nothing
 *     waits across workgroups, there are no atomics, and every loop's trip count comes from the structure.  A row of p
 *     stored entries belongs to the solves' G(p) lanes; up to [4] of the limits it is factored in LDS, beyond that by a
 *     whole wave in lu itself.
 * ------------------------------------------------------------------------------------- */
/* out: [0] default chain_rows (unmeasured: the solves' default), [1] threads of the chain workgroup, [2] longest row of
 * 4 lanes, [3] longest row of 16 lanes, [4] longest row whose working copy lives in LDS, [5] threads of a wide workgroup */
int sblas_hip_ilu0_limits(int64_t out[6]);
/* The structure check, on HOST arrays (no GPU call; testable alone), in the order given above.  diag_pos_out (n, may be
 * NULL): the position of every row's diagonal in val.  bad_row may be NULL; it is -1 on success. */
int sblas_ilu0_check(int64_t n, const int32_t *rowptr, const int32_t *colidx, int32_t *diag_pos_out, int64_t *bad_row);
/* create: copies rowptr and colidx to the host once, runs the check and the solves' host rule, and uploads every level's
 * rows packed into four-lane units, the level pointer and the diagonal positions.  Synchronises `stream`.  The plan
 * keeps the caller's rowptr / colidx POINTERS, which must outlive the plan and stay unchanged.  flags = SBLAS_SPTRSV_AUTO /
 * PER_LEVEL / CHAIN_ONLY; chain_rows: 0 = default.  bad_row may be NULL.  n == 0 succeeds. */
int sblas_hip_ilu0_plan_create(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                               int flags, int64_t chain_rows /* 0 = default */, void **plan_out, int64_t *bad_row);
/* out: [0] n [1] nnz [2] levels [3] launches [4] wide launches [5] chain launches [6] rows of the widest level [7] stored
 * entries of the longest row [8] rows on the long tier [9] device bytes held [10] flags [11] chain_rows in force */
int sblas_hip_ilu0_plan_info(const void *plan, int64_t out[12]);
/* diag_pos: a device int32[n] that lives until the plan is destroyed (NULL when n == 0): the position of each row's
 * diagonal in val and lu */
int sblas_hip_ilu0_plan_diag(const void *plan, const int32_t **diag_pos);
int sblas_hip_ilu0_plan_destroy(void *plan);
/* The factorisation.  Stream-ordered on the calling thread's current device; allocates nothing and never synchronises:
 * a fixed sequence of launches (graph-capturable as a linear chain of nodes) that takes new `val` on every call.
 * rowptr / colidx must be the pointers the plan was made with, and the current device the plan's: SBLAS_E_INVALID
 * otherwise, before anything is launched.  n == 0 succeeds and launches nothing. */
int sblas_hip_ilu0_f64_i32_planned(const void *plan, void *stream, const int32_t *rowptr, const int32_t *colidx,
                                   const double *val, double *lu);

/* ---------------------------------------------------------------------------------------
 * Multicolour reordering:  a graph colouring of a square n x n CSR pattern on the device, and the symmetric permutation
 * B = P A P^T of a CSR matrix on a plan.  int32 indices, fp64 values, n and nnz below 2^31.  Numbering the rows colour by
 * colour bounds the levels of both triangles of B by the number of colours, which is what the level-scheduled solves
 * and ILU(0) above pay for.
 *   - the graph.  u is a neighbour of v when u != v and the pattern stores (v, u) or (u, v).  The pattern need not be
 *     symmetric; rows may be unsorted, hold duplicates and lack a diagonal; diagonal entries are ignored.  A rowptr that
 *     does not start at 0, steps down or (create only, checked first, reported as row n - 1) does not end at nnz, and a
 *     column outside [0, n), are refused with SBLAS_E_INVALID and the first bad row, in the order of sblas_sptrsv_levels.
 *   - the rule, BIT-EXACT and schedule-free.  In wrapping uint32 arithmetic
 *         h(v) = fmix32((uint32)v + 0x9E3779B9u * (seed + 1u)),
 *         fmix32(x): x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
 *     fmix32 is a bijection on 32-bit words, so no two vertices tie.  Visit the vertices in descending h: color[v] is the
 *     smallest c >= 0 that no already-coloured neighbour holds.  The device runs the parallel form (Jones-Plassmann): in
 *     a round, an uncoloured vertex none of whose uncoloured neighbours has a higher h takes its first fit.  A vertex's
 *     colour depends on its neighbours of higher h alone, so both forms give the same colours whatever the schedule:
 *     color is a function of the pattern and seed.
 *   - derived arrays.  perm: the vertices sorted by (colour, vertex); inv: its inverse; color_ptr (colours + 1): class c is
 *     perm[color_ptr[c] .. color_ptr[c + 1] - 1].
 *   - consequences.  Every class is an independent set.  With B = P A P^T for this perm, the lower and the upper triangle
 *     of B each have at most `colours` levels; when the pattern is structurally symmetric each has exactly `colours`,
 *     because a vertex of colour c has a neighbour of every colour below c.
 * ------------------------------------------------------------------------------------- */
/* out: [0] longest p of 4 lanes, [1] longest p of 16 lanes (p = the stored entries of row v of A plus those of row v of
 * A^T; beyond: a whole wave), [2] colours one pass of the round kernel sees (the window), [3] threads of a round workgroup */
int sblas_hip_color_limits(int64_t out[4]);
/* The host rule, on HOST arrays (no GPU call; testable alone): the scalar loop above.  color_out[v] = the colour;
 * *n_colors = the greatest colour + 1 (0 when n == 0); *sync_rounds (may be NULL) = the rounds of the parallel form when
 * every round sees only the colours of the rounds before it.  bad_row may be NULL; it is -1 on success. */
int sblas_csr_color(int64_t n, const int32_t *rowptr, const int32_t *colidx, uint32_t seed, int32_t *color_out /* n */,
                    int64_t *n_colors, int64_t *sync_rounds, int64_t *bad_row);
/* create: copies rowptr and colidx to the host once (the check, and which lane group takes each vertex), transposes the
 * pattern on the device, runs rounds until nothing is uncoloured, and sorts by colour.  The plan owns color, perm, inv and
 * color_ptr; everything else is freed, and the caller's arrays are not kept.  Synchronises `stream`.  Rounds are separate
 * launches; nothing waits across workgroups.  The device takes at most *sync_rounds rounds; how many is not part of the
 * contract.  A round that colours nothing while vertices remain returns SBLAS_E_INTERNAL.  n == 0 succeeds. */
int sblas_hip_color_plan_create(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                                uint32_t seed, void **plan_out, int64_t *bad_row);
/* out: [0] n [1] nnz [2] colours [3] rounds [4] vertices of the largest class [5] of the smallest class [6] the largest
 * degree p (stored entries, both directions, duplicates and the diagonal counted) [7] device bytes held */
int sblas_hip_color_plan_info(const void *plan, int64_t out[8]);
/* device views that live until the plan is destroyed (any output may be NULL; all NULL when n == 0): color (n), perm (n),
 * inv (n), color_ptr (colours + 1) */
int sblas_hip_color_plan_order(const void *plan, const int32_t **color, const int32_t **perm, const int32_t **inv,
                               const int32_t **color_ptr);
int sblas_hip_color_plan_destroy(void *plan);
/* B = P A P^T for ANY permutation perm (device, n entries; row r of B is row perm[r] of A): row r of B holds the entries
 * of row perm[r] of A with columns relabelled inv[col], sorted ascending by new column, equal columns in A's stored
 * order.  A's rows may be unsorted; B's are always sorted (duplicates stay: ILU(0) still needs a pattern without them).
 * src[e] = the place in A of B's entry e.  create checks the structure (SBLAS_E_INVALID) and that perm is a permutation:
 * *bad = the first index i whose perm[i] lies outside [0, n) or repeats an earlier entry (-1 otherwise; may be NULL).
 * The plan owns rowptr_b, colidx_b, src and inv and keeps none of the caller's arrays.  Synchronises `stream`. */
int sblas_hip_permute_plan_create(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                                  const int32_t *perm, void **plan_out, int64_t *bad);
/* out: [0] n [1] nnz [2] 8-bit passes of the sort [3] device bytes held */
int sblas_hip_permute_plan_info(const void *plan, int64_t out[4]);
/* device views that live until the plan is destroyed (any output may be NULL): rowptr_b (n + 1), colidx_b (nnz), src (nnz) */
int sblas_hip_permute_plan_csr(const void *plan, const int32_t **rowptr_b, const int32_t **colidx_b, const int32_t **src);
/* inv (n; NULL when n == 0): vectors move with sblas_hip_gather_f64, x_B = x_A[perm] and x_A = x_B[inv] */
int sblas_hip_permute_plan_inverse(const void *plan, const int32_t **inv);
/* val_b[e] = val_a[src[e]].  Stream-ordered on the calling thread's current device, which must be the plan's; one launch,
 * allocates nothing, never synchronises, graph-capturable.  val_b must not overlap val_a. */
int sblas_hip_permute_plan_values(const void *plan, void *stream, const double *val_a, double *val_b);
int sblas_hip_permute_plan_destroy(void *plan);

/* ---------------------------------------------------------------------------------------
 * Krylov solvers on a plan, resident on the device:  PCG (A symmetric positive definite) and BiCGStab (A square) for
 * A x = b, fp64 values, int32 indices, with no preconditioner, Jacobi (an inverse-diagonal vector) or ILU(0) (two solve
 * plans on A's own rowptr / colidx and a factor lu).  The loop never leaves the device: the host enqueues iterations
 * and reads one scalar block back when it chooses to.
 *   - the pinned dot product.  dot(n, x, y) is two launches; nothing waits across workgroups and there are no atomics.
 *     The vector is cut into cells of C = 2048 consecutive elements, whatever the device.  A cell is summed by 256 lanes:
 *     lane t takes elements t, t + 256, ... of the cell in that order, acc = acc + x[i] * y[i] from +0 with the PRODUCT
 *     ROUNDED AND THEN THE SUM ROUNDED (no fused multiply-add); absent elements are skipped.  The 256 lane sums fold by
 *     the butterfly v[l] = v[l] + v[l ^ m] for m = 1, 2, ... 128, and lane 0's value is partial[c].  The second launch is
 *     one workgroup of W = 256 lanes: lane t adds partial[t], partial[t + 256], ... in order from +0, then the same
 *     butterfly.  So the bits are a function of n and the two vectors alone -- not of the grid, the CU count, the stream
 *     or the pointers' alignment -- and sblas_krylov_dot_ref restates them in plain C++.  (Two roundings rather than one
 *     fused multiply-add: it is ILU(0)'s rule, the kernels are bound by memory either way, and a numpy expression can
 *     restate a rounded product and a rounded sum but not a fused one.  Which NaN a sum of several NaNs returns is not
 *     part of the contract.)  n == 0 gives +0.  The multi-dot form computes up to three dots in one pass over memory;
 *     each has exactly the single dot's bits.
 *   - the updates.  Every elementwise update rounds each product and each sum on its own, in the order written:
 *       PCG       x = x + alpha * p;  r = r - alpha * q;  [Jacobi: z = dinv * r;]  p = z + beta * p
 *       BiCGStab  p = r + beta * (p - omega * v);  s = r - alpha * v;  x = (x + alpha * p^) + omega * s^;  r = s - omega * t
 *                 [Jacobi: p^ = dinv * p, s^ = dinv * s, in the pass that writes p, s]
 *     The pass that writes r is also stage 1 of (r, r) (and of (r, z) with Jacobi, of (r^, r) in BiCGStab), with the
 *     dot's order.  The scalars are read from the device scalar block; the host passes none.
 *   - the scalar step.  The single workgroup that folds a dot's cells also takes the step that follows, each operation
 *     rounded on its own:  alpha = rho / (p, q)  [BiCGStab: rho / (r^, v)],  omega = (t, s) / (t, t),  |r| = sqrt((r, r)),
 *     beta = rho_new / rho  [BiCGStab: (rho_new / rho) * (alpha / omega)],  with rho = (r, z) [BiCGStab: (r^, r)]; it
 *     evaluates  |r| <= max(rtol * |b|, atol),  counts the iteration and sets the status word:
 *     SBLAS_KRYLOV_RUNNING, _CONVERGED, _LIMIT (max_iter iterations done, test not met) or _BREAKDOWN (a denominator is
 *     zero or not finite; SBLAS_KRYLOV_DENOM_* names it).  The test comes before the limit and before beta.  BiCGStab's
 *     (t, s), (t, t) and (s, s) share one pass: when (t, t) is 0 and sqrt((s, s)) already meets the test, omega = 0 and
 *     the iteration ends as x + alpha * p^ with r = s, converged, instead of breaking down on its own success.
 *   - the freeze.  Once the status is not RUNNING the update kernels return at entry and the scalar steps change
 *     nothing: x, r, the count and |r| stay exactly those of the iteration that met the test (or of the last iteration
 *     before a breakdown), however many iterations were already enqueued.  Their SpMVs, solves and dot stages still
 *     run, into the plan's work vectors only.
 *   - edges.  n == 0: converged at iteration 0.  b == 0 (|b|^2 sums to 0): x = 0, converged at 0, nothing is divided.
 *     |r0| already within the tolerance: converged at 0, x untouched.  max_iter == 0: LIMIT at 0 unless converged.
 *     A NaN anywhere never gives CONVERGED: comparisons with it are false.
 * ------------------------------------------------------------------------------------- */
#define SBLAS_KRYLOV_PCG 0
#define SBLAS_KRYLOV_BICGSTAB 1
#define SBLAS_PRECOND_NONE 0
#define SBLAS_PRECOND_JACOBI 1
#define SBLAS_PRECOND_ILU0 2
#define SBLAS_KRYLOV_RUNNING 0
#define SBLAS_KRYLOV_CONVERGED 1
#define SBLAS_KRYLOV_BREAKDOWN 2
#define SBLAS_KRYLOV_LIMIT 3
#define SBLAS_KRYLOV_DENOM_PQ 1    /* (p, q) of PCG's alpha                  */
#define SBLAS_KRYLOV_DENOM_RHO 2   /* the previous rho, of beta              */
#define SBLAS_KRYLOV_DENOM_RV 3    /* (r^, v) of BiCGStab's alpha            */
#define SBLAS_KRYLOV_DENOM_TT 4    /* (t, t) of BiCGStab's omega             */
#define SBLAS_KRYLOV_DENOM_OMEGA 5 /* omega, of BiCGStab's beta              */
/* the fused updates of sblas_hip_krylov_update_f64 and their vectors, in order */
#define SBLAS_KRYLOV_UP_PCG_XR 0  /* x, r, p, q [, dinv, z]: partials (r, r) [, (r, z)]   */
#define SBLAS_KRYLOV_UP_PCG_P 1   /* p, z                                                  */
#define SBLAS_KRYLOV_UP_BICG_P 2  /* p, r, v [, dinv, p^]                                  */
#define SBLAS_KRYLOV_UP_BICG_S 3  /* s, r, v [, dinv, s^]                                  */
#define SBLAS_KRYLOV_UP_BICG_XR 4 /* x, r, p^, s^, s, t, r^: partials (r, r), (r^, r)      */
/* HOST functions (no GPU call; testable alone).  limits: [0] cell size C, [1] stage-2 width W (and lanes of a cell),
 * [2] work vectors of PCG, [3] of BiCGStab (ILU(0) adds the solves' temporary to either), [4] dots of one pass */
int sblas_krylov_limits(int64_t out[5]);
/* the pinned dot product restated in plain C++, on host arrays */
double sblas_krylov_dot_ref(int64_t n, const double *x, const double *y);
/* Launches of ONE iteration: the solver's own kernels, one per SpMV (a planned SpMV of k kernel classes launches k), and
 * the two solves' of every M^-1 with ILU(0) -- lower_info / upper_info are the out[12] of sblas_hip_sptrsv_plan_info
 * (read: [5] launches; NULL unless ILU(0)).  PCG: 6, with ILU(0) 8 + lower + upper.  BiCGStab: 10 + 2 (lower + upper).
 * With SBLAS_PRECOND_AMG lower_info is the out[12] of sblas_hip_amg_plan_info ([5]: launches of one cycle), upper_info is
 * not read, and the counts are ILU(0)'s with the cycle's launches as the M^-1's.  -1 for a bad argument. */
int64_t sblas_krylov_launches(int method, int precond, const int64_t *lower_info, const int64_t *upper_info);
/* The pinned dot on its own: out[k] = (x[k], y[k]) for k < ndots <= 3, one pass over memory and one fold; x, y: HOST
 * arrays of ndots device pointers, out: ndots doubles on the device.  workspace: at least ..._dot_workspace(n, ndots)
 * bytes on the device, 8-byte aligned (SBLAS_E_WORKSPACE when missing or short).  Stream-ordered, allocates nothing,
 * never synchronises, graph-capturable. */
size_t sblas_hip_krylov_dot_workspace(int64_t n, int ndots);
int sblas_hip_krylov_dot_f64(int dev, void *stream, int64_t n, int ndots, const double *const *x, const double *const *y,
                             double *out, void *workspace, size_t workspace_bytes);
/* One fused update on its own (what the solvers launch; for tests and for loops composed by the caller).  scalars: a
 * device block of 16 eight-byte slots -- [0] status as int64 (anything but SBLAS_KRYLOV_RUNNING: the call writes
 * nothing), [4] alpha, [5] beta, [6] omega as doubles.  v: a HOST array of nv device pointers in the order given at
 * SBLAS_KRYLOV_UP_*; jacobi != 0 adds dinv and the preconditioned vector.  partial: device doubles, dot k of the pass at
 * partial[k * cells + c], cells = ceil(n / C) (NULL for an update without one). */
int sblas_hip_krylov_update_f64(int dev, void *stream, int op, int jacobi, int64_t n, const double *scalars, double *const *v,
                                int nv, double *partial);
/* create: host work and one allocation (the scalar block, the partials and the work vectors).  spmv_plan: a handle of
 * sblas_hip_spmv_plan_create on the same (n, n, nnz, rowptr, colidx), or NULL for the unplanned SpMV.  precond ILU0:
 * lower_plan (SBLAS_FILL_LOWER, SBLAS_DIAG_UNIT) and upper_plan (SBLAS_FILL_UPPER, SBLAS_DIAG_NON_UNIT) of
 * sblas_hip_sptrsv_plan_create on the same rowptr / colidx; otherwise both NULL.  A plan of another device, structure,
 * fill or diag is refused (SBLAS_E_INVALID).  precond SBLAS_PRECOND_AMG: the handle of sblas_hip_amg_plan_create on the
 * same (n, nnz, rowptr, colidx) travels as lower_plan and upper_plan is NULL; it is verified with
 * sblas_hip_amg_plan_speaks_for, its cycle takes exactly the place of ILU(0)'s two solves (the same dots, folds, freeze
 * and extra work vector), and start's lu_or_dinv is ignored: the AMG plan holds its values from its own setup.  The
 * plan keeps the POINTERS and the handles, which must outlive it. */
int sblas_hip_krylov_plan_create(int dev, void *stream, int method, int64_t n, int64_t nnz, const int32_t *rowptr,
                                 const int32_t *colidx, const void *spmv_plan, int precond, const void *lower_plan,
                                 const void *upper_plan, void **plan_out);
/* out: [0] n [1] nnz [2] method [3] precond [4] work vectors owned [5] bytes of one [6] bytes of the partials [7] bytes of
 * the scalar block [8] device bytes held [9] launches of one iteration (sblas_krylov_launches) */
int sblas_hip_krylov_plan_info(const void *plan, int64_t out[10]);
int sblas_hip_krylov_plan_destroy(void *plan);
/* start: |b|, r = b - A x (A x by the SpMV, then one rounded difference), the test at iteration 0, z and the first
 * direction.  x on entry is the initial guess and is updated in place by iterate; val, lu_or_dinv (the factor for ILU0,
 * the inverse diagonal for JACOBI, ignored for NONE), b and x must stay valid and unchanged by others until the solve is
 * over.  rtol, atol >= 0, max_iter >= 0.  Stream-ordered on the calling thread's current device, which must be the
 * plan's; allocates nothing, never synchronises. */
int sblas_hip_krylov_start(void *plan, void *stream, const double *val, const double *lu_or_dinv, const double *b, double *x,
                           double rtol, double atol, int64_t max_iter);
/* iterate: enqueues k iterations.  Allocates nothing and never synchronises: a fixed linear sequence of launches
 * (graph-capturable as a chain).  SBLAS_E_INVALID before start. */
int sblas_hip_krylov_iterate(void *plan, void *stream, int64_t k);
/* status: copies the scalar block back and synchronises `stream` -- the only call of a solve that does.  out: [0]
 * status [1] iterations [2] |r| of the recurrence [3] |b| [4] alpha [5] beta [6] omega (the last of each) [7] the
 * SBLAS_KRYLOV_DENOM_* of a breakdown, else 0. */
int sblas_hip_krylov_status(const void *plan, void *stream, double out[8]);

/* ---------------------------------------------------------------------------------------
 * Restarted GMRES(m) on a plan of its own, resident on the device:  right-preconditioned GMRES for A x = b with A square,
 * fp64 values, int32 indices, restart length 1 <= m <= SBLAS_GMRES_MAX_RESTART, the preconditioners of the Krylov plan
 * (none, Jacobi, ILU(0)) and its style: start / iterate / status, only status synchronises, no atomics, nothing waits
 * across workgroups, no allocation after create, iterate is a linear graph-capturable chain, and every bit is pinned.
 * It is not a third method of sblas_hip_krylov_plan_create, which goes on refusing anything but PCG and BiCGStab.
 * One ITERATION is one Arnoldi step -- one SpMV and one M^-1 -- and max_iter counts those.
 *   - start.  |b| by the pinned dot;  r = b - A x (the SpMV, then one rounded difference);  beta = sqrt((r, r));  the test
 *     at iteration 0 with the Krylov plan's edges (b == 0: x = 0, converged at 0; |r0| within the tolerance: x untouched;
 *     max_iter == 0: LIMIT; n == 0: converged);  v_0 = r / beta, A ROUNDED DIVISION PER ELEMENT, not a multiplication by
 *     a reciprocal;  g = beta e_1.  A beta that is not finite is a BREAKDOWN (SBLAS_GMRES_DENOM_BETA), here and at a restart.
 *   - step j (0 <= j < m).  z = M^-1 v_j (Jacobi: dinv o v_j, written by the pass that writes v_j);  w = A z;  classical
 *     Gram-Schmidt done twice:  h_i = (v_i, w) for i <= j in one multi-dot pass, then w = w - h_0 v_0 - h_1 v_1 - ... - h_j v_j
 *     ascending with each product rounded and each difference rounded;  c_i = (v_i, w), h_i = h_i + c_i, and
 *     w = w - sum c_i v_i in the same order, a pass that is also stage 1 of (w, w);  eta = sqrt((w, w));  the scalar
 *     step;  v_{j+1} = w / eta, a rounded division per element.
 *   - the multi-dot.  out[i] = (V[i], w) for up to 65 columns in ONE pass over memory: a cell of the pinned dot is a
 *     workgroup, lane t keeps its eight elements of w in registers and walks the columns.  Every out[i] has exactly the
 *     bits of sblas_hip_krylov_dot_f64 on (V[i], w): the same lane order, the rounded product and then the rounded sum,
 *     the same butterfly, the same second stage (one workgroup folds the dots one after another).
 *   - the scalar step (sblas_gmres_step_ref restates it; host and device compile one text), each operation rounded on
 *     its own, in this order:  for i < j:  t = c_i h_i + s_i h_{i+1};  h_{i+1} = (-s_i) h_i + c_i h_{i+1};  h_i = t.
 *     d = sqrt(h_j h_j + eta eta).  c_j = h_j / d;  s_j = eta / d;  R_jj = d (R_ij = h_i above it).  g_{j+1} = (-s_j) g_j;
 *     g_j = c_j g_j.  The residual of the recurrence is |g_{j+1}|.  Then the iteration is counted, then the test
 *     |g_{j+1}| <= max(rtol |b|, atol), then the limit.  d zero or not finite: BREAKDOWN (SBLAS_GMRES_DENOM_GIVENS) with
 *     nothing but h changed, so the columns before j stay valid.  eta == 0 with d != 0 (the lucky breakdown) gives
 *     g_{j+1} = 0, which meets any tolerance: CONVERGED, and the division by eta never runs.  A NaN never converges.
 *   - closing a cycle forms x:  y from R y = g over the k finished columns (sblas_gmres_solve_ref: for i = k - 1 .. 0:
 *     t = g_i; for l = i + 1 .. k - 1 ascending t = t - R_il y_l; y_i = t / R_ii);  u = y_0 v_0, then u = u + y_l v_l
 *     ascending, rounded product and rounded sum;  z = M^-1 u;  x = x + z.  k is read on the device.  A close is
 *     enqueued after the m-th step of every cycle and at the end of every iterate call; it acts only when the cycle is
 *     full or the status is not RUNNING, and a correction is still unapplied, and then marks it applied.
 *   - the restart, behind the close of a full cycle while RUNNING:  r = b - A x, beta = sqrt((r, r)), the test on this
 *     true residual (it may end CONVERGED with nothing pending), the restart counted, then v_0 and g as in start.
 *   - the position.  The kernels read j from the device block, never from the launch; the host counts steps only to
 *     know where a close and a restart belong in the chain.  A step enqueued behind a full cycle (a captured chain
 *     replayed from another position) does nothing until the chain's next close and restart have run.
 *   - the freeze.  Once the status is not RUNNING, every kernel that writes x, V, g, R, c, s, the count or the status
 *     returns at entry or changes nothing, the acting close excepted: x, the count, |r| and the restart count do not
 *     depend on how many iterations were already enqueued.  max_iter stops at exactly max_iter with x formed from the
 *     columns finished so far.
 * ------------------------------------------------------------------------------------- */
#define SBLAS_GMRES_MAX_RESTART 64
#define SBLAS_GMRES_DENOM_GIVENS 6 /* d = sqrt(h_j^2 + eta^2) of a Givens rotation   */
#define SBLAS_GMRES_DENOM_BETA 7   /* |b - A x| as a cycle begins is not finite      */
/* HOST functions (no GPU call; testable alone).  limits: [0] largest restart length [1] default restart length [2]
 * columns of one multi-dot [3], [4] work vectors of a plan = [3] * m + [4] (ILU(0) adds the solves' temporary) [5] bytes of
 * the scalar block [6] bytes of the small-matrix block (R by columns, c, s, g, y, h) [7] columns whose loads one lane
 * keeps in flight together in the multi-dot */
int sblas_gmres_limits(int64_t out[8]);
/* The scalar step of Arnoldi step j (0 <= j < 64) on host arrays.  h: j + 1 entries, rotated in place; eta = |w|; c, s:
 * entries 0 .. j - 1 read, entry j written; g: entries j and j + 1 written; rcol: column j of R, j + 1 entries written;
 * tol = max(rtol |b|, atol); *iterations counted; *rnorm = |g_{j+1}|; *which = SBLAS_GMRES_DENOM_GIVENS on a breakdown,
 * which leaves everything but h as it was.  Returns the SBLAS_KRYLOV_* status, -1 for a bad argument. */
int sblas_gmres_step_ref(int j, double *h, double eta, double *c, double *s, double *g, double *rcol, double tol,
                         int64_t max_iter, int64_t *iterations, double *rnorm, int64_t *which);
/* The back substitution on host arrays: y (k entries) from R y = g, R by columns with leading dimension ldr >= k, k <= 64 */
int sblas_gmres_solve_ref(int k, const double *R, int ldr, const double *g, double *y);
/* Launches: out[0] of one step (the same for every j), out[1] of a close, out[2] of a restart, out[3] of start; counted
 * as sblas_krylov_launches counts (one per SpMV, lower_info / upper_info [5] per solve with ILU(0), NULL otherwise).
 * step 9 + lower + upper, close 3 + lower + upper, restart 4, start 6.  Returns those of a full cycle,
 * m * out[0] + out[1] + out[2], or -1 for a bad argument.  SBLAS_PRECOND_AMG: as sblas_krylov_launches (lower_info is the
 * AMG plan's info, its [5] the launches of an M^-1). */
int64_t sblas_gmres_launches(int m, int precond, const int64_t *lower_info, const int64_t *upper_info, int64_t out[4]);
/* The multi-dot on its own: out[i] = (V + i * ldv, w) for i < k <= 65; V, w, out on the device, ldv >= n when k > 1.
 * workspace: at least ..._dots_workspace(n, k) bytes on the device, 8-byte aligned (SBLAS_E_WORKSPACE when missing or
 * short).  Two launches.  Stream-ordered, allocates nothing, never synchronises, graph-capturable. */
size_t sblas_hip_gmres_dots_workspace(int64_t n, int k);
int sblas_hip_gmres_dots_f64(int dev, void *stream, int64_t n, int k, const double *V, int64_t ldv, const double *w,
                             double *out, void *workspace, size_t workspace_bytes);
/* w = w - h_0 v_0 - ... - h_{k-1} v_{k-1}, ascending, h on the device (k <= 65).  partial: NULL, or ceil(n / 2048) device
 * doubles that receive stage 1 of (w, w) over the new w.  One launch. */
int sblas_hip_gmres_project_f64(int dev, void *stream, int64_t n, int k, const double *V, int64_t ldv, const double *h,
                                double *w, double *partial);
/* u = y_0 v_0 + y_1 v_1 + ... ascending, y on the device (k <= 65); u must not overlap V.  One launch. */
int sblas_hip_gmres_combine_f64(int dev, void *stream, int64_t n, int k, const double *V, int64_t ldv, const double *y,
                                double *u);
/* create: host work and one allocation, zeroed on `stream`, which is synchronised (the two blocks, the partials,
 * V = restart + 1 columns, w, u, z [, the solves' temporary]).  spmv_plan, precond, lower_plan, upper_plan and the
 * refusals: as sblas_hip_krylov_plan_create.  The plan keeps the POINTERS and the handles, which must outlive it. */
int sblas_hip_gmres_plan_create(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                                int restart, const void *spmv_plan, int precond, const void *lower_plan,
                                const void *upper_plan, void **plan_out);
/* out: [0] n [1] nnz [2] restart [3] precond [4] work vectors owned [5] bytes of one (the column stride of V) [6] bytes of
 * the partials [7] bytes of the scalar block [8] of the small-matrix block [9] device bytes held [10] launches of a step
 * [11] of a close [12] of a restart [13] of a full cycle */
int sblas_hip_gmres_plan_info(const void *plan, int64_t out[14]);
int sblas_hip_gmres_plan_destroy(void *plan);
/* start / iterate / status: as the Krylov plan's.  iterate enqueues k steps, a close and a restart behind every m-th
 * step since start, and a close at its end.  status out: [0] status [1] iterations [2] |r| of the recurrence (|b - A x|
 * when a cycle has just begun) [3] |b| [4] restarts [5] finished columns of the open cycle [6] the last eta (beta when
 * a cycle has just begun) [7] the denominator of a breakdown, else 0. */
int sblas_hip_gmres_start(void *plan, void *stream, const double *val, const double *lu_or_dinv, const double *b, double *x,
                          double rtol, double atol, int64_t max_iter);
int sblas_hip_gmres_iterate(void *plan, void *stream, int64_t k);
int sblas_hip_gmres_status(const void *plan, void *stream, double out[8]);

/* ---------------------------------------------------------------------------------------
 * Aggregation AMG on a device plan:  z = M^-1 r by ONE V(nu, nu) cycle of a plain (unsmoothed) aggregation multigrid from
 * a zero guess, for a square CSR matrix with fp64 values and int32 indices whose rows are strictly ascending and store
 * their diagonal (ILU(0)'s structure contract and its refusal, which names the first bad row).  create works on the
 * structure, setup is numeric and repeatable, apply is a fixed graph-capturable sequence of launches that allocates
 * nothing, never synchronises, uses no atomics and in which nothing waits across workgroups.  M^-1 is symmetric when A
 * is, so PCG may use it; the Krylov and GMRES plans take the handle with SBLAS_PRECOND_AMG.  Every bit is pinned:
 *   - aggregation of level l (sblas_amg_aggregate).  The strong neighbours of row i are its stored off-diagonal
 *     entries; with values and theta > 0 only those with |a_ij| >= theta * max_{k != i} |a_ik| (the product rounded).
 *     Only row i's own entries are consulted.  The vertices are walked in descending fmix32(v + 0x9E3779B9 * (seed + l +
 *     1)) (the colouring's priority, which has no ties); a vertex is a ROOT unless one of its strong neighbours already
 *     is.  Roots are numbered in ascending vertex index; every other vertex joins the first root among its strong
 *     neighbours in stored order.  members: the vertices by (aggregate, vertex); aggptr: n_agg + 1 entries.
 *   - the coarse pattern is the COO plan (SBLAS_COO_SUM) of the triplets (agg[row(e)], agg[col(e)]) for e in stored
 *     order; the coarse values are its re-assembly: duplicates added left to right in input order.
 *   - coarsening goes on while n_l > coarse_max and l + 1 < max_levels; a level that does not reduce n is discarded.
 *     With theta > 0 the coarse levels' strength tests use coarse values formed on the host in the same order from the
 *     val given to create; the hierarchy is then fixed, and setup with other values keeps the aggregates.
 *   - setup.  wd_i = omega / a_ii (SBLAS_AMG_JACOBI, default omega 2/3) or omega / sum_e |a_ie| added sequentially in
 *     stored order from +0 (SBLAS_AMG_L1, default omega 1), a rounded division.  A diagonal that is not finite and > 0 is
 *     flagged on the device as the least (level, row); sblas_hip_amg_plan_check reads the flag and is the one call that
 *     synchronises.
 *   - the row sweep  y_i = x_i + wd_i * (b_i - s_i):  s_i is the row sum in the triangular solves' order over the whole
 *     row -- G(p) = 4 / 16 / 64 lanes for a stored length p <= 4 / <= 32 / beyond, lane l the entries l, l + G, ... with
 *     one fused multiply-add each from +0, the lanes folded by the butterfly l ^ 1, l ^ 2, ... -- then a rounded
 *     difference, a rounded product and a rounded sum.  The residual mode writes b_i - s_i; the first sweep from zero
 *     is y_i = wd_i * b_i.  x and y are distinct arrays.
 *   - restriction  b_c[I] = the residual summed over aggregate I's members in ascending vertex order, sequentially from
 *     +0;  prolongation  x_i = x_i + coarse_scale * e[agg[i]], a rounded product and a rounded sum.
 *   - a cycle on level l: nu sweeps (the first from zero), residual, restrict, the cycle of level l + 1, prolong, nu
 *     sweeps.  The coarsest level runs coarse_sweeps sweeps from zero and nothing else.  (2 nu + 3) launches a level and
 *     coarse_sweeps on the coarsest (sblas_amg_launches).
 * ------------------------------------------------------------------------------------- */
#define SBLAS_PRECOND_AMG 3
#define SBLAS_PRECOND_CHEBYSHEV 4 /* sblas_hip_cheby.h: the plan's handle in lower_plan's place, upper_plan NULL */
#define SBLAS_AMG_JACOBI 0
#define SBLAS_AMG_L1 1
#define SBLAS_AMG_CHEBYSHEV 2 /* sblas_hip_cheby.h: sblas_hip_amg_plan_setup_ex */
#define SBLAS_AMG_SWEEP 0    /* modes of sblas_hip_amg_sweep_f64 */
#define SBLAS_AMG_RESIDUAL 1
#define SBLAS_AMG_FIRST 2
/* HOST functions (no GPU call; testable alone).  limits: [0], [1] the longest stored rows that 4 and 16 lanes take [2]
 * threads of a workgroup [3] default coarse_max [4] default max_levels [5] default nu [6] default coarse_sweeps [7] the
 * largest max_levels */
int sblas_amg_limits(int64_t out[8]);
/* One level's aggregation on host arrays.  val: NULL for structure only (then theta must be 0); theta in [0, 1].  agg,
 * members: n entries; aggptr: room for n + 1, *n_agg + 1 written.  SBLAS_E_INVALID with *bad_row for a bad structure. */
int sblas_amg_aggregate(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, double theta, uint32_t seed,
                        uint32_t level, int32_t *agg, int32_t *aggptr, int32_t *members, int64_t *n_agg, int64_t *bad_row);
/* launches of one apply on `levels` levels; -1 for a bad argument (nu, coarse_sweeps >= 1; levels in [0, 64]) */
int64_t sblas_amg_launches(int levels, int nu, int coarse_sweeps);
/* setup's wd on host arrays (omega as given, no default).  *bad_row: the first row whose diagonal is not finite and > 0
 * (reported, SBLAS_OK all the same, as the device flags it), or a row without a diagonal (SBLAS_E_INVALID). */
int sblas_amg_wd_ref(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, int smoother, double omega,
                     double *wd, int64_t *bad_row);
/* The whole cycle in plain C++ on host arrays: arrays of `levels` pointers (agg, aggptr, members: levels - 1 are read; level
 * l's aggptr has n[l + 1] + 1 entries).  z must not be r. */
int sblas_amg_cycle_ref(int levels, const int64_t *n, const int32_t *const *rowptr, const int32_t *const *colidx,
                        const double *const *val, const double *const *wd, const int32_t *const *agg,
                        const int32_t *const *aggptr, const int32_t *const *members, int nu, int coarse_sweeps,
                        double coarse_scale, const double *r, double *z);
/* create: the hierarchy, host work with the device sorts of the COO plans; `stream` is synchronised.  val: device values,
 * read (once) only when theta > 0, else NULL.  coarse_max, max_levels: 0 takes the default.  Refused before any launch:
 * a bad structure (*bad_row), n or nnz beyond INT_MAX, theta outside [0, 1] or NaN, theta > 0 without val.  The plan
 * keeps the POINTERS rowptr and colidx (level 0 sweeps on them) and owns everything else. */
int sblas_hip_amg_plan_create(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                              const double *val, double theta, int64_t coarse_max, int max_levels, uint32_t seed,
                              void **plan_out, int64_t *bad_row);
/* out: [0] n [1] nnz [2] levels [3] nu [4] coarse_sweeps [5] launches of one apply [6] rows of all levels [7] stored
 * entries of all levels [8] device bytes held [9] smoother [10] 1 after a setup [11] rows of the coarsest level */
int sblas_hip_amg_plan_info(const void *plan, int64_t out[12]);
/* One level's device arrays.  sizes: [0] n [1] nnz [2] aggregates = n of the next level (0 on the coarsest) [3] four-lane
 * units of a sweep launch.  ptrs: rowptr, colidx, val, wd, agg, aggptr, members (the last three NULL on the coarsest; val
 * of level 0 is setup's pointer, NULL before it). */
int sblas_hip_amg_plan_level(const void *plan, int level, int64_t sizes[4], const void *ptrs[7]);
/* setup: every level's values and wd, device work only: allocates nothing, never synchronises, graph-capturable.
 * omega: 0 takes the smoother's default.  The plan keeps the POINTER val, which level 0 sweeps on: it must stay valid and
 * unchanged until the next setup.  Stream-ordered on the calling thread's current device, which must be the plan's. */
int sblas_hip_amg_plan_setup(void *plan, void *stream, const double *val, int smoother, double omega, int nu, int coarse_sweeps,
                             double coarse_scale);
/* apply: z = M^-1 r.  Refused before setup and when z overlaps r.  The plan owns every level vector. */
int sblas_hip_amg_plan_apply(const void *plan, void *stream, const double *r, double *z);
/* check: out[0] level, out[1] row of the least flagged diagonal of the last setup, or -1, -1; synchronises `stream` */
int sblas_hip_amg_plan_check(const void *plan, void *stream, int64_t out[2]);
/* SBLAS_OK when the plan lives on device `dev` (< 0: the current one) and was made for exactly this structure */
int sblas_hip_amg_plan_speaks_for(const void *plan, int dev, int64_t n, int64_t nnz, const int32_t *rowptr,
                                  const int32_t *colidx);
int sblas_hip_amg_plan_destroy(void *plan);
/* The single kernels on level `level` of a plan (for tests and for loops composed by the caller); one launch each.
 * sweep: mode SBLAS_AMG_SWEEP / _RESIDUAL / _FIRST (x unread), after a setup; y must overlap neither x nor b.
 * restrict: bc[I] over level `level`'s aggregates (not the coarsest level).  prolong: x_i += scale * e[agg[i]]. */
int sblas_hip_amg_sweep_f64(const void *plan, void *stream, int level, int mode, const double *b, const double *x, double *y);
int sblas_hip_amg_restrict_f64(const void *plan, void *stream, int level, const double *res, double *bc);
int sblas_hip_amg_prolong_f64(const void *plan, void *stream, int level, double scale, const double *e, double *x);

/* Smoothed aggregation on the same plan (SBLAS_AMG_SMOOTHED, sblas_hip_amg_plan_create_ex, the coarsening guard and their
 * host references) is declared in sblas_hip_amg_sa.h, which this header includes at its end; aggregation on the device
 * (sblas_hip_amg_plan_create_dev, sblas_hip_amg_aggregate_i32, sblas_amg_roots_rounds_ref) in sblas_hip_amg_dev.h, likewise;
 * the Chebyshev smoother (SBLAS_AMG_CHEBYSHEV, sblas_hip_amg_plan_setup_ex, sblas_hip_amg_plan_eig) and the plan of its own
 * (sblas_hip_cheby_plan_*, SBLAS_PRECOND_CHEBYSHEV) in sblas_hip_cheby.h, likewise. */

/* ---------------------------------------------------------------------------------------
 * SDDMM on a CSR pattern:  out[e] = alpha * <X[row(e), :], Y[col(e), :]> + beta * out[e]  for every stored entry e of A
 * (the gradient of C = A * B with respect to A's values with X = dC and Y = B; edge scores; residuals on a pattern).
 *   - A gives its PATTERN only (rowptr, colidx).  Unsorted rows and duplicate entries are legal, as everywhere else; a
 *     duplicate gets the same value twice.  rowptr is relative to the colidx / out pointers passed, so a re-based method-2
 *     row block works with X advanced to the block's first row.  out: nnz values in CSR order.
 *   - X is rows x k, Y is cols x k: row c of Y is what entry (r, c) is multiplied with.  In the cuSPARSE / rocSPARSE
 *     wording (C = alpha * (A * B) o spy(C) + beta * C with B of shape k x cols) Y is B transposed: a row-major B is a
 *     column-major Y with the same leading dimension, a column-major B a row-major Y.
 *   - orders and leading dimensions as in sblas_hip_spmm_csr_ordered: SBLAS_ROW_MAJOR X[r * ldx + j] (ldx >= k),
 *     SBLAS_COL_MAJOR X[r + j * ldx] (ldx >= rows, for Y ldy >= cols).  A row-major operand is read in place with 64-bit
 *     offsets: 16-byte loads when both bases are 16-byte aligned and both leading dimensions even, 8-byte loads
 *     otherwise (same bits).  A column-major operand is first copied row-major into the workspace by the SpMM staging
 *     copy (64-bit addressing, no size limit of its own); sblas_hip_sddmm_csr_workspace is 0 when both are row-major and
 *     grows only with the column-major ones.  workspace: 16-byte aligned.
 *   - columns k .. ld - 1 of a row-major operand and whatever lies behind its last row are never loaded.
 *   - beta == 0: out is not read (a NaN in it does not survive), as for C in SpMM.  alpha == 0 is no shortcut, as in
 *     SpMM: the dot product is formed and multiplied, so NaN / Inf in the operands reach out.
 *   - k == 0: out = alpha * 0 + beta * out (the operands may be NULL).  nnz == 0 (and with it rows == 0, cols == 0)
 *     launches nothing.  A bad order, a leading dimension below its minimum, a missing pointer: SBLAS_E_INVALID; a
 *     missing or short workspace: SBLAS_E_WORKSPACE; both before anything touches the device.
 *   - stream-ordered, allocates nothing, never synchronises, graph-capturable.  SBLAS_VALIDATE=1 checks the structure
 *     first (synchronises), as for SpMM.
 *   - summation order: a function of k alone.  The bits of out[e] depend only on the k values of the two operand rows,
 *     on k, alpha, beta and the old out[e] -- not on where e sits, its row's length, its neighbours, the operands'
 *     orders, leading dimensions or alignment, or the run.  No floating-point atomics.  k is cut into slices of 128
 *     elements (the last one shorter); a slice of kj elements is summed by G = 1, 2, 4, 8, 16 lanes for kj <= 4, 8,
 *     32, 64, more: lane l adds the products of elements 2q, 2q + 1 for q = l, l + G, l + 2G, ... in that order, one fma
 *     each, from +0; the G sums are folded s += s[l ^ 1], s += s[l ^ 2], s += s[l ^ 4], s += s[l ^ 8].  The first slice
 *     gives out = alpha * s, or fma(beta, out, alpha * s); every later slice out = out + alpha * s.
 * fp64 values and int32 indices only.
 * ------------------------------------------------------------------------------------- */
size_t sblas_hip_sddmm_csr_workspace(int64_t rows, int64_t cols, int64_t nnz, int64_t k, int order_x, int order_y);
int sblas_hip_sddmm_csr_f64_i32(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz,
                                const int32_t *rowptr, const int32_t *colidx,
                                const double *X, int64_t ldx, int order_x,
                                const double *Y, int64_t ldy, int order_y,
                                int64_t k, double alpha, double beta, double *out,
                                void *workspace, size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------
 * Row-wise softmax on a CSR pattern (edge softmax) and its backward.  For every row, over its stored entries e in
 * stored order:
 *     forward    t[e] = scale * x[e],  m = max t,  s = sum exp(t[e] - m),  out[e] = exp(t[e] - m) / s
 *     backward   d = sum p[e] * dp[e],  dx[e] = (scale * p[e]) * (dp[e] - d)        (p: the forward's output)
 *   - only the pattern's rowptr is read; colidx is not an argument.  Unsorted rows and duplicate entries are ordinary
 *     entries.  An empty row costs nothing and writes nothing.  out may be x; dx may be dp.
 *   - rowptr is relative to the value pointers passed: a row-aligned block of a larger matrix (rows [r0, r1), row
 *     pointers re-based to start at 0, the value pointers advanced to the block's first entry) gives the bits of the
 *     whole call.  A block of sblas_partition_nnz is NOT a valid input when it cuts a row (it may): the softmax of a
 *     piece of a row is not a piece of the row's softmax.
 *   - workspace: sblas_hip_csr_softmax_workspace(rows, nnz) bytes, 16-byte aligned; it depends on rows and nnz alone and
 *     is 0 when no row can exceed 4096 entries (nnz <= 4096).  It holds per-call partial results of rows longer than
 *     that, nothing that outlives the call; forward and backward may share it.
 *   - nnz == 0 launches nothing.  A missing pointer, a negative size, entries with rows == 0: SBLAS_E_INVALID; a missing
 *     or short workspace: SBLAS_E_WORKSPACE (misaligned: SBLAS_E_INVALID); all before anything touches the device.
 *   - stream-ordered, allocates nothing, never synchronises, graph-capturable.  SBLAS_VALIDATE=1 first checks that
 *     rowptr starts at 0, never descends and ends at nnz (synchronises); a bad one is SBLAS_E_INVALID, nothing written.
 *   - IEEE classes, those of torch.softmax on each row: a NaN anywhere in a row makes the whole row NaN (the max
 *     propagates NaN); -Inf entries get +0 when the row has a finite entry; a row whose max is +Inf is NaN, so is a row
 *     of -Inf only; scale == 0 is no shortcut (0 * Inf reaches the row); exp underflowing to subnormal or 0 is ordinary.
 *   - summation order: a function of the row's length L alone.  The bits of out[e] depend only on the row's values in
 *     stored order, on L and on scale -- not on which row it is, where its entries sit in the value array, the
 *     neighbouring rows, workgroup boundaries, the run, or which kernel took the row.  No floating-point atomics.  With
 *     the row's entries numbered 0 .. L - 1: leaf i is exp(t[i] - m) (backward: fma(p[i], dp[i], +0)); a cell is the 64
 *     leaves from a multiple of 64, absent ones +0, folded v += v[l ^ 1], v += v[l ^ 2], v += v[l ^ 4], v += v[l ^ 8],
 *     v += v[l ^ 16], v += v[l ^ 32]; a supercell is 64 cells from a multiple of 64, absent ones +0, their sums folded
 *     the same way; the row sum is +0 plus the supercell sums, left to right.  scale * x, t - m, the division,
 *     scale * p, dp - d and the last product are each rounded once (nothing is contracted into an fma).
 * fp64 values and int32 row pointers only.
 * ------------------------------------------------------------------------------------- */
size_t sblas_hip_csr_softmax_workspace(int64_t rows, int64_t nnz);
int sblas_hip_csr_softmax_f64_i32(int dev, void *stream, int64_t rows, int64_t nnz, const int32_t *rowptr,
                                  const double *x, double scale, double *out, void *workspace, size_t workspace_bytes);
int sblas_hip_csr_softmax_backward_f64_i32(int dev, void *stream, int64_t rows, int64_t nnz, const int32_t *rowptr,
                                           const double *p, const double *dp, double scale, double *dx,
                                           void *workspace, size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------
 * Fused attention on a CSR pattern and its backward.  For every row i, over its stored entries e in stored order, with
 * c(e) = colidx[e]:
 *     forward    s[e] = <Q[i, :], K[c(e), :]> (d elements),  t = scale * s,  m = max t,  z = sum exp(t - m),
 *                p[e] = exp(t[e] - m) / z,  O[i, :] = sum_e p[e] V[c(e), :] (dv elements),  row_max[i] = m, row_sum[i] = z
 *     backward   t, p again from Q, K, row_max, row_sum;  dp[e] = <dO[i, :], V[c(e), :]>,  D = sum_e p[e] dp[e],
 *                dS[e] = (scale * p[e]) * (dp[e] - D),  dQ[i, :] = sum_e dS[e] K[c(e), :];  P and dS on request
 *   - Q rows x d, K cols x d, V cols x dv, O / dO rows x dv, dQ rows x d: row-major, leading dimension >= width, any
 *     alignment; elements beyond the width in a row are never read.  1 <= d, dv <= 128.  Anything else: SBLAS_E_INVALID.
 *   - the forward writes no nnz-sized array.  row_max / row_sum (rows doubles each): both or neither; NULL for inference.
 *     The backward writes dQ, P (nnz) and dS (nnz), each only when its pointer is not NULL, and does no work for what is
 *     not asked (P alone forms no dp).  dK = A(dS)^T Q and dV = A(P)^T dO are the caller's transposed products.
 *   - rows of every length, no plan, no host look at the structure.  workspace:
 *     sblas_hip_csr_attention_workspace(rows, nnz, d, dv) bytes, 16-byte aligned, 0 when nnz <= 4096; it holds the
 *     per-supercell figures and partial rows of rows longer than 4096 entries (about nnz / 4096 rows of max(d, dv)),
 *     nothing that outlives the call; forward and backward may share it.
 *   - an empty row: O[i, :] = +0, row_max = -Inf, row_sum = +0, dQ[i, :] = +0; nnz == 0 still writes those rows.
 *   - argument checks come before anything touches the device (SBLAS_E_INVALID; SBLAS_E_WORKSPACE for a missing or short
 *     workspace); stream-ordered, allocates nothing, never synchronises, graph-capturable.  SBLAS_VALIDATE=1 checks
 *     rowptr and colidx first (synchronises).
 *   - bits: P and dS are those of sblas_hip_csr_softmax_f64_i32 on sblas_hip_sddmm_csr_f64_i32's scores (alpha 1, beta 0)
 *     and of the softmax backward on the SDDMM of dO and V.  O[i, :] and dQ[i, :] depend on Q[i, :] (dO[i, :]), the rows
 *     of K and V the row's entries name in stored order, the row's length, d, dv and scale only -- not on the row's
 *     index or place, its neighbours, leading dimensions, alignment or the kernel that took it.  With W the power of two
 *     in [4, 64] covering min(width, 64) output columns and NG = 64 / W: inside a run (a row of up to 4096 entries, or
 *     4096 entries of a longer row counted from its start) entry j goes to accumulator j % NG, which starts at +0 and
 *     takes acc = fma(p[j], V[c(j), c], acc) in ascending j; the NG accumulators fold acc += acc[g ^ 1], acc[g ^ 2], ...;
 *     a longer row is +0 plus its runs' rows, left to right.  No floating-point atomics.
 *   - IEEE classes follow from those expressions: p == 0 and scale == 0 are no shortcut, a NaN row of P gives a NaN row
 *     of O.
 * fp64 values and int32 indices only.
 * ------------------------------------------------------------------------------------- */
size_t sblas_hip_csr_attention_workspace(int64_t rows, int64_t nnz, int64_t d, int64_t dv);
int sblas_hip_csr_attention_f64_i32(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz,
                                    const int32_t *rowptr, const int32_t *colidx,
                                    const double *Q, int64_t ldq, const double *K, int64_t ldk, const double *V, int64_t ldv,
                                    int64_t d, int64_t dv, double scale, double *O, int64_t ldo,
                                    double *row_max, double *row_sum, void *workspace, size_t workspace_bytes);
int sblas_hip_csr_attention_backward_f64_i32(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz,
                                             const int32_t *rowptr, const int32_t *colidx,
                                             const double *Q, int64_t ldq, const double *K, int64_t ldk,
                                             const double *V, int64_t ldv, int64_t d, int64_t dv, double scale,
                                             const double *dO, int64_t lddo, const double *row_max, const double *row_sum,
                                             double *dQ, int64_t lddq, double *P, double *dS,
                                             void *workspace, size_t workspace_bytes);

/* sblas_partition_nnz (below) for 64-bit row pointers */
int64_t sblas_partition_nnz_i64(const int64_t *rowptr, int64_t rows, int64_t nnz, int n_gpu, int i_gpu,
                                int64_t *start_row, int64_t *stop_row, int64_t *nnz_i, int64_t *first_nnz,
                                int64_t *rebased_rowptr);

/* ---------------------------------------------------------------------------------------
 * Host-side placement arithmetic (pure functions, no GPU needed).
 * ------------------------------------------------------------------------------------- */
/* csr_findRowIdxUsingNnzIdx, utility.h:292-300 (same answer, O(log M)). */
int32_t sblas_find_row_of_nnz(const int32_t *rowptr, int32_t rows, int32_t nnz_idx);

/* nnz-balanced row-block partition of CsrSparseMatrix::sync2gpu(segment), matrix.h:356-375.
 * Uses the exact integer ceil((nnz)/g) (the reference's float ceil drops nonzeros above 2^24;
 * both agree below).  rebased_rowptr may be NULL; otherwise it must hold stop-start+2 ints.
 * Returns the number of row pointers (stop_row - start_row + 2) or a negative value. */
int64_t sblas_partition_nnz(const int32_t *rowptr, int32_t rows, int32_t nnz, int n_gpu, int i_gpu,
                            int32_t *start_row, int32_t *stop_row, int32_t *nnz_i,
                            int64_t *first_nnz, int32_t *rebased_rowptr);

/* Leading-dimension block partition of DenseMatrix::sync2gpu(segment), matrix.h:554-568. */
int sblas_partition_dense(int64_t first_order, int n_gpu, int i_gpu,
                          int64_t *offset, int64_t *dim);

/* The SpMV plan's classifier (sblas_hip_spmv_plan_create runs it on a host copy of rowptr).  Cuts rows [0, rows) into
 * work items of at most one kernel block of consecutive rows, four int32 each: first row, row count, kind
 * (SBLAS_SPMV_ITEM_*), pieces (split items only, else 0).  Items come in row order and cover every row exactly once.
 * nnz sets the matrix average the unplanned launcher would use.  split_min / piece <= 0 take the defaults below; a row
 * with more than split_min nonzeros becomes a split item of ceil(len / piece) pieces.  Writes up to max_items items
 * when `items` is not NULL and returns the number of items, or -1 (bad argument, descending row pointers). */
#define SBLAS_SPMV_ITEM_LPR 0        /* lanes-per-row kernel, 4 lanes per row (64 rows per item)     */
#define SBLAS_SPMV_ITEM_STREAM4096 1 /* stream kernel, 4096 products of LDS (256 rows)               */
#define SBLAS_SPMV_ITEM_STREAM6144 2 /* stream kernel, 6144 products of LDS (256 rows)               */
#define SBLAS_SPMV_ITEM_SEG 3        /* segmented kernel, four rows per wave (16 rows)               */
#define SBLAS_SPMV_ITEM_LDS_S2 4     /* LDS-window kernel, 2 / 3 / 4 / 7 slices in flight (8 rows)   */
#define SBLAS_SPMV_ITEM_LDS_S3 5
#define SBLAS_SPMV_ITEM_LDS_S4 6
#define SBLAS_SPMV_ITEM_LDS_S7 7
#define SBLAS_SPMV_ITEM_SPLIT 8      /* one long row, cut into pieces                                */
#define SBLAS_SPMV_SPLIT_MIN 12288   /* default: rows longer than two 6144-product stream runs       */
#define SBLAS_SPMV_SPLIT_PIECE 4096  /* default nonzeros per piece (one 256-thread workgroup)        */
int64_t sblas_spmv_plan_classify(const int32_t *rowptr, int64_t rows, int64_t nnz, int64_t split_min, int64_t piece,
                                 int32_t *items, int64_t max_items);

/* The split SpMM plan's classifier (sblas_hip_spmm_plan_create_split runs it on host copies of rowptr and the panel
 * verdicts).  A row is split when it has at least split_min nonzeros and its panel is one the plan gives to the direct
 * kernels: direct_mask holds one byte per panel of panel_rows rows (nonzero: direct), NULL means every panel.  A split
 * row of len nonzeros becomes ceil(len / piece) pieces of consecutive nonzeros, at most `piece` each.  Records of four
 * int32: first the pieces {row, first nonzero, end, partial slot} with slots 0, 1, .. in row order (the pieces of a row
 * consecutive, in CSR order), then one record per split row {row, first slot, pieces, -1}.  split_min / piece <= 0
 * take the defaults below.  Writes up to max_out records when `out` is not NULL and returns the number of records
 * (pieces + split rows), or -1 (bad argument, row pointers descending or outside [0, nnz]). */
#define SBLAS_SPMM_SPLIT_MIN 16384   /* default: rows of this many nonzeros or more are split        */
#define SBLAS_SPMM_SPLIT_PIECE 4096  /* default nonzeros per piece (one 1024-thread workgroup)       */
int64_t sblas_spmm_split_classify(const int32_t *rowptr, int64_t rows, int64_t nnz, int64_t split_min, int64_t piece,
                                  const uint8_t *direct_mask, int64_t panel_rows, int32_t *out, int64_t max_out);

/* The SpMM kernel rule as a host function (no GPU): what one column chunk of an SpMM call of these sizes does -- how B
 * is staged, where the panel verdicts come from, the panel geometry, and which stage-2 kernels are launched with which
 * template arguments, in launch order -- under the environment switches as last read (sblas_hip_debug_reload_env).
 * ldbt is the staged width (sblas_hip_spmm_ldbt), n <= ldbt the chunk's columns, ncu the device's compute units.
 * caller_staged != 0: the call of sblas_hip_spmm_csr_rowmajorB_f64_i32.  plan: NULL for an unplanned call, else the
 * SBLAS_SPMM_RULE_PLAN_FIELDS counts of a plan (sblas_hip_spmm_plan_info / _split_info) the rule reads.  Writes up to
 * max_out of the SBLAS_SPMM_RULE_FIELDS values when `out` is not NULL and returns SBLAS_SPMM_RULE_FIELDS, or -1 (bad
 * argument). */
enum {
    SBLAS_SPMM_RULE_PLAN_N_WINDOW = 0, /* panels of the LDS-tiled kernel                                   */
    SBLAS_SPMM_RULE_PLAN_N_DIRECT,     /* ... of the direct kernels                                        */
    SBLAS_SPMM_RULE_PLAN_N_MFMA_W,     /* ... of the matrix-core kernel, falling back to the LDS-tiled one */
    SBLAS_SPMM_RULE_PLAN_N_MFMA_D,     /* ... falling back to the direct kernels                           */
    SBLAS_SPMM_RULE_PLAN_MERGE,        /* the vote gave the direct panels to the row-merging kernel        */
    SBLAS_SPMM_RULE_PLAN_FOUR_ROWS,    /* ... to the four-rows-per-wave kernel                             */
    SBLAS_SPMM_RULE_PLAN_N_SPLIT,      /* split rows (a split plan)                                        */
    SBLAS_SPMM_RULE_PLAN_PANEL_ROWS,   /* panel height                                                     */
    SBLAS_SPMM_RULE_PLAN_GROUPS,       /* groups of four rows per wave                                     */
    SBLAS_SPMM_RULE_PLAN_FIELDS
};
enum {
    /* stage 1 */
    SBLAS_SPMM_RULE_STAGING = 0,     /* 0 caller's Bt, 1 whole B, 2 whole B + classifier in one launch, 3 column range, 4 planned */
    SBLAS_SPMM_RULE_VERDICTS,        /* 0 none, 1 from the staging launch, 2 a launch of their own, 3 an earlier chunk's, 4 the plan's */
    SBLAS_SPMM_RULE_PANEL_ROWS,      /* panel height (1: nothing classified)                              */
    SBLAS_SPMM_RULE_GROUPS,          /* groups of four rows per wave                                      */
    SBLAS_SPMM_RULE_PANELS,          /* classified panels                                                 */
    SBLAS_SPMM_RULE_PLANNABLE,       /* sblas_hip_spmm_plan_create would keep the verdicts                */
    /* stage 2, in launch order; 0 = not launched */
    SBLAS_SPMM_RULE_TILED,           /* 1 spmm_window6_kernel<G, NH>, 2 spmm_lanes_kernel<NC, CP, G, LPE> */
    SBLAS_SPMM_RULE_TILED_G,
    SBLAS_SPMM_RULE_W6_NH,
    SBLAS_SPMM_RULE_W6_GRID_Y,       /* workgroups along the dense columns                                */
    SBLAS_SPMM_RULE_LANES_NC,
    SBLAS_SPMM_RULE_LANES_CP,
    SBLAS_SPMM_RULE_LANES_LPE,
    SBLAS_SPMM_RULE_MFMA,            /* the matrix-core kernel ...                                        */
    SBLAS_SPMM_RULE_MFMA_BATCH,      /* ... operand blocks per stage                                      */
    SBLAS_SPMM_RULE_MFMA_LDS_FLOOR,  /* ... least dynamic LDS, bytes                                      */
    SBLAS_SPMM_RULE_FOUR_ROWS,       /* four-rows-per-wave direct kernel ...                              */
    SBLAS_SPMM_RULE_FOUR_ROWS_WAVES, /* ... waves per workgroup                                           */
    SBLAS_SPMM_RULE_FOUR_ROWS_VOTED, /* ... 1: runs only where the device-side vote says so               */
    SBLAS_SPMM_RULE_MERGE,           /* row-merging direct kernel                                         */
    SBLAS_SPMM_RULE_DPP_GROUPS,      /* row-per-wave direct kernel: its GROUPS (1, 2, 4) ...              */
    SBLAS_SPMM_RULE_DPP_PAD,         /* ... dynamic LDS pad, bytes                                        */
    SBLAS_SPMM_RULE_DPP_LONG,        /* ... entries from which the whole workgroup computes a row         */
    SBLAS_SPMM_RULE_NARROW,          /* lane-group direct kernel: 8, 16 or 32 columns                     */
    SBLAS_SPMM_RULE_ROWS8,           /* wave-per-row direct kernel of 8 columns                           */
    SBLAS_SPMM_RULE_INTERLEAVE,      /* panel map of the direct kernels: 1 interleave, 0 contiguous, -1 by span */
    SBLAS_SPMM_RULE_SKIP,            /* a split plan: SKIP instantiations, then the split kernels ...     */
    SBLAS_SPMM_RULE_SPLIT_GROUPS,    /* ... with this GROUPS                                              */
    SBLAS_SPMM_RULE_FIELDS
};
int64_t sblas_spmm_rule_describe(int64_t rows, int64_t cols, int64_t nnz, int64_t ldbt, int64_t n, int64_t ncu,
                                 int caller_staged, const int64_t *plan, int64_t *out, int64_t max_out);

/* Dense initialiser of the reference's DenseMatrix(h, w, order) / DenseVector(len) constructors (matrix.h:519-528,
 * :663-672; utility.h:197; config.h:23 seed 211): srand(seed), then rand() / RAND_MAX in storage order (host memory). */
int sblas_host_fill_rand0to1(double *dst, int64_t count, unsigned seed);

/* ---------------------------------------------------------------------------------------
 * MatrixMarket -> CSR (host).  Same observable result as mmio_info / mmio_data
 * (mmio_highlevel.h:7-127, :130-281): file order preserved inside a row, symmetric/hermitian
 * mirrored, skew treated as general, pattern -> 1.0, complex -> real part, 1-based -> 0-based.
 * Single pass over the text, arrays sized by the caller from sblas_mm_read_info.
 * ------------------------------------------------------------------------------------- */
int sblas_mm_read_info(const char *path, int32_t *rows, int32_t *cols, int32_t *nnz,
                       int32_t *is_symmetric);
int sblas_mm_read_csr(const char *path, int32_t *rowptr, int32_t *colidx, double *val);

#ifdef __cplusplus
}
#endif
#include "sblas_hip_amg_sa.h"
#include "sblas_hip_amg_dev.h"
#include "sblas_hip_cheby.h"
#include "sblas_hip_krylov_multi.h"
#include "sblas_hip_amg_multi.h"
#include "sblas_hip_sptrsm_tile.h"
#include "sblas_hip_gmres_multi.h"
#include "sblas_hip_geam.h"
#include "sblas_hip_mspgemm.h"
#include "sblas_hip_sddmm_narrow.h"
#include "sblas_hip_fsai.h"
#include "sblas_hip_eigsh.h"
#endif /* SBLAS_HIP_H */
