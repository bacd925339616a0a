// transpose.hip -- A^T on the device: CSR -> CSC (sblas_hip_csr_transpose_f64_i32), the value gather that refreshes it
// (sblas_hip_gather_f64) and the transpose plan whose products run the existing planned SpMV / SpMM on the CSC arrays.
//
// The CSC order is fixed: column c lists its entries in CSR order (ascending row, duplicates as stored), which is what a
// stable sort of the column indices gives.  The sort is an LSD radix sort of the colidx keys with the nonzero index k as
// payload, one 8-bit digit per pass and only as many passes as cols - 1 has bytes:
//   hist    one workgroup per tile of 4096 keys counts its digits (wave-private counters in LDS, no atomics);
//   scan    exclusive scan of the digit-major histogram (digit d of tile t at d * tiles + t): every key's destination
//           base is the count of smaller digits plus the same digit in earlier tiles;
//   scatter the same tile ranks each key among the keys of its digit: a wave finds the lanes holding its digit with eight
//           ballots, its rank is the number of those lanes below it, and per-wave running counters in LDS (seeded with
//           the earlier waves' counts) carry the rank across the wave's 16 rounds.  Keys go out in (round, lane) order
//           of each wave's contiguous 1024 keys, so every pass is stable.
// Then colptr[c] = the number of sorted keys below c (a binary search per column: no scan over cols, no atomics), and
// one pass over the nonzeros writes perm[i] = k, rowidx[i] = row(k) (binary search in rowptr) and valT[i] = val[k].
// Nothing depends on scheduling: the same input gives the same bits on every run.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <memory>
#include "../../include/sblas_hip.h"
#include "capi_util.h"
#include "kernels.h"
#include "radix_sort.h"

namespace {

// position i of the CSC arrays: nonzero k = sidx[i] (identity when no pass ran) of row r, rowptr[r] <= k < rowptr[r + 1]
__global__ __launch_bounds__(T_THREADS) void transpose_finish_kernel(const int32_t *__restrict__ sidx, int64_t nnz,
                                                                     const int32_t *__restrict__ rowptr, int64_t rows,
                                                                     const double *__restrict__ val, int32_t *__restrict__ rowidx,
                                                                     double *__restrict__ valT, int32_t *__restrict__ perm)
{
    for (int64_t i = (int64_t)blockIdx.x * T_THREADS + threadIdx.x; i < nnz; i += (int64_t)gridDim.x * T_THREADS) {
        const int32_t k = sidx ? sidx[i] : (int32_t)i;
        int64_t lo = 0, hi = rows - 1; // the last row whose start is <= k (empty rows share their start with the next)
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (rowptr[mid] <= k) lo = mid;
            else hi = mid - 1;
        }
        rowidx[i] = (int32_t)lo;
        if (valT) valT[i] = val[k];
        if (perm) perm[i] = k;
    }
}

hipError_t run_transpose(hipStream_t s, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                         const double *val, int32_t *colptr, int32_t *rowidx, double *valT, int32_t *perm, void *workspace)
{
    const int32_t *skeys = colidx, *sidx = nullptr;
    if (nnz > 0) {
        Workspace w;
        workspace_layout(nnz, static_cast<char *>(workspace), &w);
        const int passes = radix_passes(cols);
        for (int p = 0; p < passes; ++p) {
            const hipError_t e = radix_pass(s, w, skeys, sidx, nnz, p * RADIX_BITS, p & 1);
            if (e != hipSuccess) return e;
            skeys = w.keys[p & 1], sidx = w.idx[p & 1];
        }
    }
    colptr_kernel<<<grid_for(cols + 1), T_THREADS, 0, s>>>(skeys, nnz, cols, nullptr, colptr);
    if (nnz > 0)
        transpose_finish_kernel<<<grid_for(nnz), T_THREADS, 0, s>>>(sidx, nnz, rowptr, rows, val, rowidx, valT, perm);
    return hipGetLastError();
}

// the transpose's host-side argument checks (SBLAS_OK, SBLAS_E_INVALID or SBLAS_E_WORKSPACE)
int transpose_args(int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr, const int32_t *colidx, const double *val,
                   const int32_t *colptr, const int32_t *rowidx, const double *valT, const void *workspace, size_t workspace_bytes)
{
    if (rows < 0 || cols < 0 || nnz < 0 || rows > INT_MAX || cols > INT_MAX || nnz > INT_MAX) return SBLAS_E_INVALID;
    if (!rowptr || !colptr) return SBLAS_E_INVALID;
    if (nnz > 0 && (!colidx || !rowidx || (val == nullptr) != (valT == nullptr))) return SBLAS_E_INVALID;
    if (nnz > 0 && (rows == 0 || cols == 0)) return SBLAS_E_INVALID; // no row / column to hold a nonzero
    const size_t need = sblas_hip_csr_transpose_workspace(rows, cols, nnz);
    if (need > 0 && (!workspace || workspace_bytes < need)) return SBLAS_E_WORKSPACE;
    if (!aligned16(workspace)) return SBLAS_E_INVALID;
    return SBLAS_OK;
}

// A plan: A^T as CSR in buffers of its own, the SpMV plan over them and, for a width n > 0, an SpMM plan.
struct TransposePlan {
    int dev = -1;
    int64_t rows = 0, cols = 0, nnz = 0, n = 0;
    DeviceBuffer buf; // colptr | rowidx | valT | perm
    size_t bytes = 0;
    int32_t *colptr = nullptr, *rowidx = nullptr, *perm = nullptr;
    double *valT = nullptr;
    void *spmv = nullptr, *spmm = nullptr;
    ~TransposePlan()
    {
        sblas_hip_spmv_plan_destroy(spmv);
        sblas_hip_spmm_plan_destroy(spmm);
    }
};

} // namespace

extern "C" {

size_t sblas_hip_csr_transpose_workspace(int64_t rows, int64_t cols, int64_t nnz)
{
    if (rows < 0 || cols < 0 || nnz <= 0 || nnz > INT_MAX || radix_passes(cols) == 0) return 0;
    return workspace_layout(nnz, nullptr, nullptr);
}

int sblas_hip_csr_transpose_f64_i32(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr,
                                    const int32_t *colidx, const double *val, int32_t *colptr, int32_t *rowidx, double *valT,
                                    int32_t *perm, void *workspace, size_t workspace_bytes)
{
    if (const int rc = transpose_args(rows, cols, nnz, rowptr, colidx, val, colptr, rowidx, valT, workspace, workspace_bytes))
        return rc;
    if (sblas::options().validate && rows > 0 && nnz > 0) {
        const int vrc = sblas_hip_debug_validate_csr_i32(dev, stream, rows, cols, nnz, rowptr, colidx);
        if (vrc) return vrc;
    }
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    return run_transpose((hipStream_t)stream, rows, cols, nnz, rowptr, colidx, val, colptr, rowidx, valT, perm, workspace) ==
                   hipSuccess
               ? SBLAS_OK
               : SBLAS_E_HIP;
}

int sblas_hip_gather_f64(int dev, void *stream, int64_t n, const int32_t *idx, const double *src, double *dst)
{
    if (n < 0) return SBLAS_E_INVALID;
    if (n == 0) return SBLAS_OK;
    if (!idx || !src || !dst) return SBLAS_E_INVALID;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    gather_f64_kernel<<<grid_for(n), T_THREADS, 0, (hipStream_t)stream>>>(n, idx, src, dst);
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_transpose_plan_create(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr,
                                    const int32_t *colidx, const double *val, int64_t n, int flags, void **plan_out)
{
    if (!plan_out) return SBLAS_E_INVALID;
    *plan_out = nullptr;
    // A^T has cols rows: the SpMV / SpMM entry points take at most INT_MAX - 64 of them
    if (rows < 0 || cols < 0 || nnz < 0 || n < 0 || rows > INT_MAX || cols > INT_MAX - 64 || nnz > INT_MAX || n > INT_MAX)
        return SBLAS_E_INVALID;
    if (!rowptr || (nnz > 0 && (!colidx || !val)) || (flags & ~SBLAS_TRANSPOSE_SPLIT) != 0) return SBLAS_E_INVALID;
    if (nnz > 0 && (rows == 0 || cols == 0)) return SBLAS_E_INVALID;
    std::unique_ptr<TransposePlan> p(new TransposePlan);
    p->dev = resolve_device(dev), p->rows = rows, p->cols = cols, p->nnz = nnz, p->n = n;
    if (cols == 0) { // A^T has no rows: every product is empty, nothing is held on the device
        *plan_out = p.release();
        return SBLAS_OK;
    }
    // the transpose kernels never see a column index outside [0, cols)
    if (rows > 0) {
        const int vrc = sblas_hip_debug_validate_csr_i32(dev, stream, rows, cols, nnz, rowptr, colidx);
        if (vrc) return vrc;
    }
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    hipStream_t s = (hipStream_t)stream;
    const size_t cp = align16(((size_t)cols + 1) * sizeof(int32_t)), ri = align16((size_t)nnz * sizeof(int32_t));
    const size_t vt = align16((size_t)nnz * sizeof(double));
    p->bytes = cp + ri + vt + ri;
    if (p->buf.alloc(p->dev, p->bytes) != hipSuccess) return SBLAS_E_HIP;
    p->colptr = p->buf.at<int32_t>(), p->rowidx = p->buf.at<int32_t>(cp);
    p->valT = p->buf.at<double>(cp + ri), p->perm = p->buf.at<int32_t>(cp + ri + vt);
    {
        const size_t wsb = sblas_hip_csr_transpose_workspace(rows, cols, nnz);
        DeviceBuffer ws; // freed before the sub-plans are made
        if (wsb > 0 && ws.alloc(p->dev, wsb) != hipSuccess) return SBLAS_E_HIP;
        hipError_t e = run_transpose(s, rows, cols, nnz, rowptr, colidx, val, p->colptr, p->rowidx, p->valT, p->perm, ws.at<void>());
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return SBLAS_E_HIP;
    }
    int rc = sblas_hip_spmv_plan_create(dev, stream, cols, rows, nnz, p->colptr, p->rowidx, &p->spmv);
    if (rc == SBLAS_OK && n > 0)
        rc = (flags & SBLAS_TRANSPOSE_SPLIT)
                 ? sblas_hip_spmm_plan_create_split(dev, stream, cols, rows, nnz, p->colptr, p->rowidx, n, 0, 0, &p->spmm)
                 : sblas_hip_spmm_plan_create(dev, stream, cols, rows, nnz, p->colptr, p->rowidx, n, &p->spmm);
    if (rc != SBLAS_OK) return rc;
    *plan_out = p.release();
    return SBLAS_OK;
}

int sblas_hip_transpose_plan_destroy(void *plan)
{
    delete static_cast<TransposePlan *>(plan);
    return SBLAS_OK;
}

int sblas_hip_transpose_plan_update_values(void *plan, void *stream, const double *val)
{
    if (!plan) return SBLAS_E_INVALID;
    const TransposePlan *p = static_cast<const TransposePlan *>(plan);
    if (p->nnz == 0) return SBLAS_OK;
    if (!val) return SBLAS_E_INVALID;
    return sblas_hip_gather_f64(p->dev, stream, p->nnz, p->perm, val, p->valT);
}

int sblas_hip_transpose_plan_info(const void *plan, int64_t out[8])
{
    if (!plan || !out) return SBLAS_E_INVALID;
    const TransposePlan *p = static_cast<const TransposePlan *>(plan);
    int64_t sv[8] = {0}, sm[4] = {0};
    if (p->spmv) sblas_hip_spmv_plan_info(p->spmv, sv);
    if (p->spmm) sblas_hip_spmm_plan_split_info(p->spmm, sm);
    out[0] = (bool)p->buf, out[1] = p->nnz, out[2] = (int64_t)p->bytes, out[3] = p->spmm != nullptr;
    out[4] = p->spmm ? p->n : 0, out[5] = sv[6], out[6] = sm[0], out[7] = 0;
    return SBLAS_OK;
}

int sblas_hip_transpose_plan_csc(const void *plan, const int32_t **colptr, const int32_t **rowidx, const double **valT)
{
    if (!plan) return SBLAS_E_INVALID;
    const TransposePlan *p = static_cast<const TransposePlan *>(plan);
    if (colptr) *colptr = p->colptr;
    if (rowidx) *rowidx = p->rowidx;
    if (valT) *valT = p->valT;
    return SBLAS_OK;
}

int sblas_hip_spmv_csr_t_f64_i32_planned(const void *plan, int dev, void *stream, const double *x, double alpha, double beta,
                                         double *y)
{
    if (!plan) return SBLAS_E_INVALID;
    const TransposePlan *p = static_cast<const TransposePlan *>(plan);
    if (p->dev != resolve_device(dev)) return SBLAS_E_INVALID;
    if ((p->cols > 0 && !y) || (p->rows > 0 && !x)) return SBLAS_E_INVALID;
    if (p->cols == 0) return SBLAS_OK;
    return sblas_hip_spmv_csr_f64_i32_planned(p->spmv, dev, stream, p->cols, p->rows, p->nnz, p->colptr, p->rowidx, p->valT, x,
                                              alpha, beta, y);
}

int sblas_hip_spmm_csr_t_f64_i32_planned(const void *plan, int dev, void *stream, const double *B, int64_t ldb, int order_b,
                                         int64_t n, double alpha, double beta, double *C, int64_t ldc, int order_c,
                                         void *workspace, size_t workspace_bytes)
{
    if (!plan || !order_ok(order_b) || !order_ok(order_c) || n < 0) return SBLAS_E_INVALID;
    const TransposePlan *p = static_cast<const TransposePlan *>(plan);
    if (p->dev != resolve_device(dev)) return SBLAS_E_INVALID;
    if (n == 0) return SBLAS_OK;
    // A^T's shape: B is rows x n, C is cols x n
    if (!C || !ld_ok(order_c, ldc, p->cols, n)) return SBLAS_E_INVALID;
    if (p->rows > 0 && (!B || !ld_ok(order_b, ldb, p->rows, n))) return SBLAS_E_INVALID;
    if (p->cols == 0) return SBLAS_OK;
    const size_t need = p->nnz > 0 ? sblas_hip_spmm_csr_f64_i32_workspace(p->cols, p->rows, p->nnz, n) : 0;
    if (need > 0 && (!workspace || workspace_bytes < need)) return SBLAS_E_WORKSPACE;
    if (p->spmm && n == p->n)
        return sblas_hip_spmm_csr_ordered_f64_i32_planned(p->spmm, dev, stream, p->cols, p->rows, p->nnz, p->colptr, p->rowidx,
                                                          p->valT, B, ldb, order_b, n, alpha, beta, C, ldc, order_c, workspace,
                                                          workspace_bytes);
    return sblas_hip_spmm_csr_ordered(dev, stream, SBLAS_F64, SBLAS_I32, p->cols, p->rows, p->nnz, p->colptr, p->rowidx, p->valT,
                                      B, ldb, order_b, n, alpha, beta, C, ldc, order_c, workspace, workspace_bytes);
}

} // extern "C"
