// coo.hip -- CSR on the device from unsorted COO triplets (sblas_hip_coo_to_csr_f64_i32) and the assembly plan that sorts
// a fixed structure once and turns new triplet values into CSR values with one launch (sblas_hip_coo_plan_*).
//
// The order is fixed: entries sorted by (row, col), equal pairs in input order -- numpy.lexsort((col, row)).  The sort is
// transpose.hip's stable LSD radix sort (radix_sort.h) with the triplet index as payload: the column digits first, then
// the row digits, so ceil(bits(cols - 1) / 8) + ceil(bits(rows - 1) / 8) passes.  Between the two halves one gather
// writes the row keys in the column-sorted order.  Then
//   KEEP  rowptr[r] = the number of sorted row keys below r (a binary search per row: no scan over rows, no atomics) and
//         one pass writes colidx[i] = col[k], val[i] = coo_val[k], perm[i] = k, runptr[i] = i for k = the payload of i;
//   SUM   heads   marks[i] = 1 where (row, col) differs from position i - 1, and the sorted columns;
//         scan    exclusive scan of the marks (nnz + 1 of them, the last is 0, so its scanned value is the entry count);
//         rowptr  rowptr[r] = the scanned mark count at row r's lower bound (colptr_kernel with the counts);
//         compact a head at position i with e heads before it writes colidx[e] and runptr[e] = i;
//         sum     val[e] = ((v1 + v2) + v3) + ... over coo_val[perm[k]], k in [runptr[e], runptr[e + 1]), by one lane.
// The sum kernel is the plan's repeated hot path.  A workgroup owns 256 consecutive entries, whose runs are one
// contiguous range of sorted positions: all 256 threads read perm and gather the values of a 2048-position chunk into
// LDS (coalesced perm reads, every gather independent of every add), then each lane adds its own run from LDS in input
// order.  No floating-point atomics and nothing that depends on scheduling: the same input gives the same bits on
// every run.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <memory>
#include "../../include/sblas_hip.h"
#include "capi_util.h"
#include "kernels.h"
#include "radix_sort.h"
#include "coo_sum.h"

namespace {

// flag[0] = 1 when a triplet lies outside [0, rows) x [0, cols)
__global__ __launch_bounds__(T_THREADS) void coo_validate_kernel(int64_t nnz, int64_t rows, int64_t cols,
                                                                 const int32_t *__restrict__ row, const int32_t *__restrict__ col,
                                                                 int *__restrict__ flag)
{
    int bad = 0;
    for (int64_t k = (int64_t)blockIdx.x * T_THREADS + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * T_THREADS) {
        const int32_t r = row[k], c = col[k];
        if (r < 0 || (int64_t)r >= rows || c < 0 || (int64_t)c >= cols) bad = 1;
    }
    if (bad) atomicOr(flag, bad);
}

// reads every index once and waits for the answer; nothing else runs on the triplets before it is known
hipError_t validate_coo(hipStream_t s, int64_t rows, int64_t cols, int64_t nnz, const int32_t *row, const int32_t *col, int *bad)
{
    int *flag = nullptr;
    hipError_t e = hipMalloc(&flag, sizeof(int));
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(flag, 0, sizeof(int), s);
    if (e == hipSuccess) {
        coo_validate_kernel<<<grid_for(nnz), T_THREADS, 0, s>>>(nnz, rows, cols, row, col, flag);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(bad, flag, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(flag);
    return e;
}

// the longest run (plan info): an integer maximum, the same whatever the order
__global__ __launch_bounds__(T_THREADS) void coo_longest_run_kernel(int64_t entries, const int32_t *__restrict__ runptr,
                                                                    int *__restrict__ longest)
{
    int m = 0;
    for (int64_t e = (int64_t)blockIdx.x * T_THREADS + threadIdx.x; e < entries; e += (int64_t)gridDim.x * T_THREADS) {
        const int len = runptr[e + 1] - runptr[e];
        m = len > m ? len : m;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const int y = __shfl_down(m, o, 64);
        m = y > m ? y : m;
    }
    if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(longest, m);
}

// the size checks every COO entry point shares: sizes below 2^31, a known mode, a place for every triplet
bool coo_shape_ok(int64_t rows, int64_t cols, int64_t nnz, int dup)
{
    if (rows < 0 || cols < 0 || nnz < 0 || rows > INT_MAX || cols > INT_MAX || nnz > INT_MAX) return false;
    if (dup != SBLAS_COO_KEEP && dup != SBLAS_COO_SUM) return false;
    return !(nnz > 0 && (rows == 0 || cols == 0));
}

// An assembly plan: the sorted structure of one set of (row, col) triplets in buffers of its own.
struct CooPlan {
    int dev = -1, dup = SBLAS_COO_KEEP;
    int64_t rows = 0, cols = 0, nnz = 0, csr_nnz = 0, longest = 0, passes = 0;
    DeviceBuffer buf; // rowptr | colidx | perm | runptr
    size_t bytes = 0;
    int32_t *rowptr = nullptr, *colidx = nullptr, *perm = nullptr, *runptr = nullptr;
};

} // namespace

extern "C" {

size_t sblas_hip_coo_to_csr_workspace(int64_t rows, int64_t cols, int64_t nnz)
{
    if (rows < 0 || cols < 0 || nnz <= 0 || nnz > INT_MAX) return 0;
    return coo_layout(nnz, nullptr, nullptr);
}

int sblas_hip_coo_to_csr_f64_i32(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz, const int32_t *coo_row,
                                 const int32_t *coo_col, const double *coo_val, int dup, int32_t *rowptr, int32_t *colidx,
                                 double *val, int32_t *perm, int32_t *runptr, void *workspace, size_t workspace_bytes)
{
    if (!coo_shape_ok(rows, cols, nnz, dup) || !rowptr) return SBLAS_E_INVALID;
    if (nnz > 0 && (!coo_row || !coo_col || !colidx || (coo_val == nullptr) != (val == nullptr))) return SBLAS_E_INVALID;
    const size_t need = sblas_hip_coo_to_csr_workspace(rows, cols, nnz);
    if (need > 0 && (!workspace || workspace_bytes < need)) return SBLAS_E_WORKSPACE;
    if (!aligned16(workspace)) return SBLAS_E_INVALID;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    hipStream_t s = (hipStream_t)stream;
    if (sblas::options().validate && nnz > 0) {
        int bad = 0;
        if (validate_coo(s, rows, cols, nnz, coo_row, coo_col, &bad) != hipSuccess) return SBLAS_E_HIP;
        if (bad) return SBLAS_E_INVALID;
    }
    return run_coo(s, rows, cols, nnz, coo_row, coo_col, coo_val, dup, rowptr, colidx, val, perm, runptr, workspace) == hipSuccess
               ? SBLAS_OK
               : SBLAS_E_HIP;
}

int sblas_hip_coo_plan_create(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz, const int32_t *coo_row,
                              const int32_t *coo_col, int dup, void **plan_out)
{
    if (!plan_out) return SBLAS_E_INVALID;
    *plan_out = nullptr;
    if (!coo_shape_ok(rows, cols, nnz, dup) || (nnz > 0 && (!coo_row || !coo_col))) return SBLAS_E_INVALID;
    std::unique_ptr<CooPlan> p(new CooPlan);
    p->dev = resolve_device(dev), p->dup = dup, p->rows = rows, p->cols = cols, p->nnz = nnz;
    p->passes = nnz > 0 ? radix_passes(cols) + radix_passes(rows) : 0;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    hipStream_t s = (hipStream_t)stream;
    if (nnz > 0) { // the sort kernels never see an index outside [0, rows) x [0, cols)
        int bad = 0;
        if (validate_coo(s, rows, cols, nnz, coo_row, coo_col, &bad) != hipSuccess) return SBLAS_E_HIP;
        if (bad) return SBLAS_E_INVALID;
    }
    const size_t rp = align16(((size_t)rows + 1) * sizeof(int32_t)), ar = align16(((size_t)nnz + 1) * sizeof(int32_t));
    p->bytes = rp + 3 * ar;
    if (p->buf.alloc(p->dev, p->bytes) != hipSuccess) return SBLAS_E_HIP;
    p->rowptr = p->buf.at<int32_t>(), p->colidx = p->buf.at<int32_t>(rp);
    p->perm = p->buf.at<int32_t>(rp + ar), p->runptr = p->buf.at<int32_t>(rp + 2 * ar);
    int32_t count = 0;
    int longest = 0;
    {
        const size_t wsb = sblas_hip_coo_to_csr_workspace(rows, cols, nnz);
        DeviceBuffer ws; // the sort workspace, freed when the structure stands
        if (wsb > 0 && ws.alloc(p->dev, wsb) != hipSuccess) return SBLAS_E_HIP;
        hipError_t e = run_coo(s, rows, cols, nnz, coo_row, coo_col, nullptr, dup, p->rowptr, p->colidx, nullptr, p->perm,
                               p->runptr, ws.at<void>());
        if (e == hipSuccess) e = hipMemcpyAsync(&count, p->rowptr + rows, sizeof(count), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e == hipSuccess && dup == SBLAS_COO_SUM && count > 0) { // the workspace's first word holds the maximum
            int *d = ws.at<int>();
            e = hipMemsetAsync(d, 0, sizeof(int), s);
            if (e == hipSuccess) {
                coo_longest_run_kernel<<<grid_for(count), T_THREADS, 0, s>>>(count, p->runptr, d);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipMemcpyAsync(&longest, d, sizeof(int), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
        } else if (count > 0) {
            longest = 1;
        }
        if (e != hipSuccess) return SBLAS_E_HIP;
    }
    p->csr_nnz = count, p->longest = longest;
    *plan_out = p.release();
    return SBLAS_OK;
}

int sblas_hip_coo_plan_destroy(void *plan)
{
    delete static_cast<CooPlan *>(plan);
    return SBLAS_OK;
}

int sblas_hip_coo_plan_info(const void *plan, int64_t out[8])
{
    if (!plan || !out) return SBLAS_E_INVALID;
    const CooPlan *p = static_cast<const CooPlan *>(plan);
    out[0] = p->rows, out[1] = p->cols, out[2] = p->nnz, out[3] = p->csr_nnz, out[4] = p->longest, out[5] = p->passes;
    out[6] = (int64_t)p->bytes, out[7] = p->dup;
    return SBLAS_OK;
}

int sblas_hip_coo_plan_csr(const void *plan, const int32_t **rowptr, const int32_t **colidx, const int32_t **perm,
                           const int32_t **runptr)
{
    if (!plan) return SBLAS_E_INVALID;
    const CooPlan *p = static_cast<const CooPlan *>(plan);
    if (rowptr) *rowptr = p->rowptr;
    if (colidx) *colidx = p->colidx;
    if (perm) *perm = p->perm;
    if (runptr) *runptr = p->runptr;
    return SBLAS_OK;
}

int sblas_hip_coo_plan_assemble(const void *plan, void *stream, const double *coo_val, double *val_out)
{
    if (!plan) return SBLAS_E_INVALID;
    const CooPlan *p = static_cast<const CooPlan *>(plan);
    if (p->nnz == 0) return SBLAS_OK;
    if (!coo_val || !val_out) return SBLAS_E_INVALID;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID; // the plan's arrays live on its own device
    hipStream_t s = (hipStream_t)stream;
    if (p->dup == SBLAS_COO_KEEP)
        gather_f64_kernel<<<grid_for(p->nnz), T_THREADS, 0, s>>>(p->nnz, p->perm, coo_val, val_out);
    else
        coo_assemble_sum_kernel<<<grid_for(p->csr_nnz), T_THREADS, 0, s>>>(p->rowptr + p->rows, p->runptr, p->perm, coo_val,
                                                                          val_out);
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

} // extern "C"
