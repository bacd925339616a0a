// mspgemm.hip -- masked SpGEMM out = M o (X * Y^T) on the device (sblas_hip_mspgemm_plan_*): create checks the three
// structures, decides the path and copies them into the plan with the row of every mask entry beside them; numeric is one
// launch over the mask's entries, a lane each.  The contract ((V), (I), (D), (S)) stands above the declarations in
// sblas_hip_mspgemm.h; the host restatement is mspgemm_rule.cpp.
//
// The sorted path (every row of X and of Y strictly ascending).  A workgroup takes 256 consecutive mask entries, so a
// mask row of a million entries is 4000 ordinary workgroups.  The lane of entry (i, j) walks the shorter of X's row i and
// Y's row j and finds each of its columns in the longer by a binary search that starts where the last one ended:
// O(min log max), and the matches come in ascending shared column, which with unique columns on both sides is (V)'s
// order.  The entries a wave holds mostly share i: the wave stages the X row its first entry names, columns and values, in
// its own 3 KiB of LDS when that row has at most MSPGEMM_LDS_ROW entries; lanes of that row walk or search the copy, the
// others (a wave that straddles rows, a longer row) read global memory.  Y's rows are gathered.  Which side is walked
// and where X's row is read from change no bit: the products and their order are the same.
// The general path (any row of X or Y unsorted or with a duplicate, or SBLAS_MSPGEMM_GENERAL), the slow one: the lane walks
// X's row in stored order and for each entry Y's row in stored order -- (V) word for word, len(X row) * len(Y row)
// comparisons an entry.
// No atomics in numeric, no scratch, nothing waits across workgroups.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <memory>
#include "../../include/sblas_hip.h"
#include "capi_util.h"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function" // radix_sort.h's sort passes, scans and gathers: not used here
#include "radix_sort.h"                              // T_THREADS, grid_for, ceil_div, align16
#pragma clang diagnostic pop
#include "mspgemm.h"
#include "rowwise.h" // block_row_of

// x * y and p1 + p2 are separate roundings
#pragma clang fp contract(off)

namespace {

using sblas::MSPGEMM_LDS_ROW;
using sblas::MSPGEMM_THREADS;
using sblas::MSPGEMM_WAVES;
static_assert(MSPGEMM_THREADS == T_THREADS, "grid_for counts workgroups of T_THREADS");

// rowptr[0] == 0 and no step down: flag |= 1
__global__ __launch_bounds__(MSPGEMM_THREADS) void mspgemm_rowptr_check_kernel(int64_t rows, const int32_t *__restrict__ rowptr,
                                                                               int *__restrict__ flag)
{
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * MSPGEMM_THREADS + threadIdx.x; i < rows; i += (int64_t)gridDim.x * MSPGEMM_THREADS) {
        if (rowptr[i + 1] < rowptr[i]) bad = 1;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && rowptr[0] != 0) bad = 1;
    if (bad) atomicOr(flag, 1);
}

// a column outside [0, cols): flag |= 1
__global__ __launch_bounds__(MSPGEMM_THREADS) void mspgemm_colidx_check_kernel(int64_t nnz, int64_t cols, const int32_t *__restrict__ colidx,
                                                                               int *__restrict__ flag)
{
    int bad = 0;
    for (int64_t p = (int64_t)blockIdx.x * MSPGEMM_THREADS + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * MSPGEMM_THREADS) {
        const int32_t c = colidx[p];
        if (c < 0 || (int64_t)c >= cols) bad = 1;
    }
    if (bad) atomicOr(flag, 1);
}

// One pass over the entries of a checked structure (rows >= 1, nnz >= 1), one workgroup per 256 of them, all threads
// present for the block-wide searches.  row_out (the mask): row_out[e] = the row of entry e.  flag (X and Y): |= 1 for an
// entry that does not lie strictly above its predecessor in the same row.
__global__ __launch_bounds__(MSPGEMM_THREADS) void mspgemm_entry_pass_kernel(int rows, int nnz, const int32_t *__restrict__ rowptr,
                                                                             const int32_t *__restrict__ colidx, int32_t *__restrict__ row_out,
                                                                             int *__restrict__ flag)
{
    const int64_t e0 = (int64_t)blockIdx.x * MSPGEMM_THREADS, e = e0 + threadIdx.x;
    const int64_t e1 = e0 + MSPGEMM_THREADS - 1 < nnz - 1 ? e0 + MSPGEMM_THREADS - 1 : nnz - 1;
    int lo = sblas::block_row_of<MSPGEMM_THREADS>(rowptr, rows, (int)e0);
    int hi = sblas::block_row_of<MSPGEMM_THREADS>(rowptr, rows, (int)e1);
    if (e >= nnz) return;
    while (lo < hi) { // the largest r in [lo, hi] with rowptr[r] <= e
        const int mid = (int)(((int64_t)lo + hi + 1) >> 1);
        if (rowptr[mid] <= (int32_t)e) lo = mid;
        else hi = mid - 1;
    }
    if (row_out) row_out[e] = lo;
    if (flag && e > rowptr[lo] && colidx[e] <= colidx[e - 1]) atomicOr(flag, 1);
}

// the first position in [p0, p1) of an ascending run of columns that holds a column >= c; p1 when there is none
template <typename Cols> __device__ __forceinline__ int32_t lower_bound_col(Cols colidx, int32_t p0, int32_t p1, int32_t c)
{
    while (p0 < p1) {
        const int32_t mid = p0 + ((p1 - p0) >> 1);
        if (colidx[mid] < c) p0 = mid + 1;
        else p1 = mid;
    }
    return p0;
}

// (V)'s running sum: the first product is copied, each later one added
struct Sum {
    double acc = 0.0; // no pair: +0.0
    bool first = true;
    __device__ __forceinline__ void add(double p)
    {
        acc = first ? p : acc + p;
        first = false;
    }
};

// The intersection of two ascending rows, the products in ascending shared column.  (wc, wv, wn): the walked row, columns,
// values and length; (sc, sv, sn): the searched one.  Which of the two is X's does not matter: x * y and y * x round alike.
template <typename WCols, typename WVals, typename SCols, typename SVals>
__device__ __forceinline__ double intersect(WCols wc, WVals wv, int32_t wn, SCols sc, SVals sv, int32_t sn)
{
    Sum s;
    int32_t lo = 0;
    for (int32_t q = 0; q < wn && lo < sn; ++q) {
        const int32_t c = wc[q];
        lo = lower_bound_col(sc, lo, sn, c);
        if (lo < sn && sc[lo] == c) {
            s.add(wv[q] * sv[lo]);
            ++lo;
        }
    }
    return s.acc;
}

// the sorted path: out[t] for the 256 mask entries of the workgroup
__global__ __launch_bounds__(MSPGEMM_THREADS) void mspgemm_sorted_kernel(int64_t nnz_m, const int32_t *__restrict__ mrow,
                                                                         const int32_t *__restrict__ colidx_m, const int32_t *__restrict__ rowptr_x,
                                                                         const int32_t *__restrict__ colidx_x, const double *__restrict__ val_x,
                                                                         const int32_t *__restrict__ rowptr_y, const int32_t *__restrict__ colidx_y,
                                                                         const double *__restrict__ val_y, double *__restrict__ out)
{
    __shared__ double s_val[MSPGEMM_WAVES][MSPGEMM_LDS_ROW];
    __shared__ int32_t s_col[MSPGEMM_WAVES][MSPGEMM_LDS_ROW];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t t0 = (int64_t)blockIdx.x * MSPGEMM_THREADS + wave * 64, t = t0 + lane;
    int32_t staged_row = -1; // the X row in this wave's LDS
    if (t0 < nnz_m) {
        const int32_t i0 = mrow[t0], p0 = rowptr_x[i0], len = rowptr_x[i0 + 1] - p0;
        if (len <= MSPGEMM_LDS_ROW) {
            staged_row = i0;
            for (int32_t q = lane; q < len; q += 64) s_col[wave][q] = colidx_x[p0 + q], s_val[wave][q] = val_x[p0 + q];
        }
    }
    __syncthreads();
    if (t >= nnz_m) return;
    const int32_t i = mrow[t], j = colidx_m[t];
    const int32_t x0 = rowptr_x[i], xn = rowptr_x[i + 1] - x0, y0 = rowptr_y[j], yn = rowptr_y[j + 1] - y0;
    const int32_t *xc = colidx_x + x0, *yc = colidx_y + y0;
    const double *xv = val_x + x0, *yv = val_y + y0;
    double r;
    if (i == staged_row) {
        r = xn <= yn ? intersect(s_col[wave], s_val[wave], xn, yc, yv, yn) : intersect(yc, yv, yn, s_col[wave], s_val[wave], xn);
    } else {
        r = xn <= yn ? intersect(xc, xv, xn, yc, yv, yn) : intersect(yc, yv, yn, xc, xv, xn);
    }
    out[t] = r;
}

// the general path: (V) as it is written, a lane per mask entry
__global__ __launch_bounds__(MSPGEMM_THREADS) void mspgemm_general_kernel(int64_t nnz_m, const int32_t *__restrict__ mrow,
                                                                          const int32_t *__restrict__ colidx_m, const int32_t *__restrict__ rowptr_x,
                                                                          const int32_t *__restrict__ colidx_x, const double *__restrict__ val_x,
                                                                          const int32_t *__restrict__ rowptr_y, const int32_t *__restrict__ colidx_y,
                                                                          const double *__restrict__ val_y, double *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * MSPGEMM_THREADS + threadIdx.x;
    if (t >= nnz_m) return;
    const int32_t i = mrow[t], j = colidx_m[t];
    const int32_t x1 = rowptr_x[i + 1], y0 = rowptr_y[j], y1 = rowptr_y[j + 1];
    Sum s;
    for (int32_t e = rowptr_x[i]; e < x1; ++e) {
        const int32_t c = colidx_x[e];
        const double x = val_x[e];
        for (int32_t g = y0; g < y1; ++g)
            if (colidx_y[g] == c) s.add(x * val_y[g]);
    }
    out[t] = s.acc;
}

struct MspgemmPlan {
    int dev = -1, flags = 0, path = SBLAS_MSPGEMM_PATH_SORTED;
    int64_t m = 0, n = 0, k = 0, nnz_m = 0, nnz_x = 0, nnz_y = 0, x_ascending = 0, y_ascending = 0;
    size_t bytes = 0;
    DeviceBuffer structure; // mrow | colidx_m | rowptr_x | colidx_x | rowptr_y | colidx_y
    const int32_t *mrow = nullptr, *colidx_m = nullptr, *rowptr_x = nullptr, *colidx_x = nullptr, *rowptr_y = nullptr, *colidx_y = nullptr;
};

// one workgroup per 256 entries, all of them present: the entry pass's searches are block-wide
inline unsigned entry_grid(int64_t nnz) { return (unsigned)ceil_div(nnz, MSPGEMM_THREADS); }

// One structure's checks: rowptr (rows + 1 entries) starts at 0 and never steps down, *nnz = rowptr[rows], and every
// column lies in [0, cols).  *bad says whether it failed; the columns are not read when the rowptr did.
hipError_t check_structure(hipStream_t s, int64_t rows, int64_t cols, const int32_t *rowptr, const int32_t *colidx, int *flag, int *bad,
                           int32_t *nnz)
{
    *bad = 0, *nnz = 0;
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), s);
    if (e != hipSuccess) return e;
    mspgemm_rowptr_check_kernel<<<grid_for(rows), MSPGEMM_THREADS, 0, s>>>(rows, rowptr, flag);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(bad, flag, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(nnz, rowptr + rows, sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess || *bad || *nnz == 0) return e;
    if (!colidx) {
        *bad = 1;
        return hipSuccess;
    }
    mspgemm_colidx_check_kernel<<<grid_for(*nnz), MSPGEMM_THREADS, 0, s>>>(*nnz, cols, colidx, flag); // the flag is still 0
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(bad, flag, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
}

// *ascending = every row of the checked structure is strictly ascending
hipError_t check_ascending(hipStream_t s, int64_t rows, int64_t nnz, const int32_t *rowptr, const int32_t *colidx, int *flag, int64_t *ascending)
{
    *ascending = 1;
    if (nnz < 2) return hipSuccess;
    int bad = 0;
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), s);
    if (e != hipSuccess) return e;
    mspgemm_entry_pass_kernel<<<entry_grid(nnz), MSPGEMM_THREADS, 0, s>>>((int)rows, (int)nnz, rowptr, colidx, nullptr, flag);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    *ascending = bad ? 0 : 1;
    return e;
}

} // namespace

extern "C" {

int sblas_hip_mspgemm_plan_create(int dev, void *stream, int64_t m, int64_t n, int64_t k, const int32_t *rowptr_m, const int32_t *colidx_m,
                                  const int32_t *rowptr_x, const int32_t *colidx_x, const int32_t *rowptr_y, const int32_t *colidx_y, int flags,
                                  void **plan_out)
{
    if (!plan_out) return SBLAS_E_INVALID;
    *plan_out = nullptr;
    if (m < 0 || n < 0 || k < 0 || m > INT_MAX - 64 || n > INT_MAX - 64 || k > INT_MAX) return SBLAS_E_INVALID;
    if (flags != SBLAS_MSPGEMM_AUTO && flags != SBLAS_MSPGEMM_GENERAL) return SBLAS_E_INVALID;
    if (!rowptr_m || !rowptr_x || !rowptr_y) return SBLAS_E_INVALID;
    std::unique_ptr<MspgemmPlan> p(new MspgemmPlan);
    p->dev = resolve_device(dev), p->flags = flags, p->m = m, p->n = n, p->k = k;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    hipStream_t s = (hipStream_t)stream;

    // the checks: nothing follows an index before it is known to be in range
    DeviceBuffer small; // a flag
    if (small.alloc(p->dev, 16) != hipSuccess) return SBLAS_E_HIP;
    int *flag = small.at<int>();
    int bad = 0;
    int32_t nnz_m = 0, nnz_x = 0, nnz_y = 0;
    if (check_structure(s, m, n, rowptr_m, colidx_m, flag, &bad, &nnz_m) != hipSuccess) return SBLAS_E_HIP;
    if (bad) return SBLAS_E_INVALID;
    if (check_structure(s, m, k, rowptr_x, colidx_x, flag, &bad, &nnz_x) != hipSuccess) return SBLAS_E_HIP;
    if (bad) return SBLAS_E_INVALID;
    if (check_structure(s, n, k, rowptr_y, colidx_y, flag, &bad, &nnz_y) != hipSuccess) return SBLAS_E_HIP;
    if (bad) return SBLAS_E_INVALID;
    p->nnz_m = nnz_m, p->nnz_x = nnz_x, p->nnz_y = nnz_y;

    // one pass over each colidx: strictly ascending rows or not
    if (check_ascending(s, m, nnz_x, rowptr_x, colidx_x, flag, &p->x_ascending) != hipSuccess) return SBLAS_E_HIP;
    if (check_ascending(s, n, nnz_y, rowptr_y, colidx_y, flag, &p->y_ascending) != hipSuccess) return SBLAS_E_HIP;
    p->path = (flags != SBLAS_MSPGEMM_GENERAL && p->x_ascending && p->y_ascending) ? SBLAS_MSPGEMM_PATH_SORTED : SBLAS_MSPGEMM_PATH_GENERAL;

    // the plan's copies, and the row of every mask entry
    const size_t b_m = align16((size_t)nnz_m * 4 + 4), b_x = align16((size_t)nnz_x * 4 + 4), b_y = align16((size_t)nnz_y * 4 + 4);
    const size_t b_rx = align16(((size_t)m + 1) * 4), b_ry = align16(((size_t)n + 1) * 4);
    const size_t o_cm = b_m, o_rx = o_cm + b_m, o_cx = o_rx + b_rx, o_ry = o_cx + b_x, o_cy = o_ry + b_ry, total = o_cy + b_y;
    if (p->structure.alloc(p->dev, total) != hipSuccess) return SBLAS_E_HIP;
    p->bytes = total;
    int32_t *mrow = p->structure.at<int32_t>();
    p->mrow = mrow, p->colidx_m = p->structure.at<int32_t>(o_cm), p->rowptr_x = p->structure.at<int32_t>(o_rx);
    p->colidx_x = p->structure.at<int32_t>(o_cx), p->rowptr_y = p->structure.at<int32_t>(o_ry), p->colidx_y = p->structure.at<int32_t>(o_cy);
    const struct {
        const int32_t *dst, *src;
        size_t count;
    } copies[5] = {{p->colidx_m, colidx_m, (size_t)nnz_m}, {p->rowptr_x, rowptr_x, (size_t)m + 1}, {p->colidx_x, colidx_x, (size_t)nnz_x},
                   {p->rowptr_y, rowptr_y, (size_t)n + 1}, {p->colidx_y, colidx_y, (size_t)nnz_y}};
    hipError_t e = hipSuccess;
    for (int c = 0; c < 5 && e == hipSuccess; ++c)
        if (copies[c].count) e = hipMemcpyAsync(const_cast<int32_t *>(copies[c].dst), copies[c].src, copies[c].count * 4, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && nnz_m > 0) {
        mspgemm_entry_pass_kernel<<<entry_grid(nnz_m), MSPGEMM_THREADS, 0, s>>>((int)m, (int)nnz_m, rowptr_m, colidx_m, mrow, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s); // the caller's arrays are read until here
    else (void)hipStreamSynchronize(s);               // no copy is in flight when the plan's buffer goes
    if (e != hipSuccess) return SBLAS_E_HIP;
    *plan_out = p.release();
    return SBLAS_OK;
}

int sblas_hip_mspgemm_plan_info(const void *plan, int64_t out[12])
{
    if (!plan || !out) return SBLAS_E_INVALID;
    const MspgemmPlan *p = static_cast<const MspgemmPlan *>(plan);
    out[0] = p->m, out[1] = p->n, out[2] = p->k, out[3] = p->nnz_m, out[4] = p->nnz_x, out[5] = p->nnz_y;
    out[6] = p->path, out[7] = p->x_ascending, out[8] = p->y_ascending;
    out[9] = p->nnz_m == 0 ? 0 : sblas::MSPGEMM_LAUNCHES;
    out[10] = (int64_t)p->bytes, out[11] = p->flags;
    return SBLAS_OK;
}

int sblas_hip_mspgemm_plan_numeric(const void *plan, void *stream, const double *val_x, const double *val_y, double *out)
{
    if (!plan) return SBLAS_E_INVALID;
    const MspgemmPlan *p = static_cast<const MspgemmPlan *>(plan);
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID; // the plan's arrays live on its own device
    if (p->nnz_m == 0) return SBLAS_OK;
    if (!out || (p->nnz_x > 0 && !val_x) || (p->nnz_y > 0 && !val_y)) return SBLAS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (p->path == SBLAS_MSPGEMM_PATH_SORTED)
        mspgemm_sorted_kernel<<<entry_grid(p->nnz_m), MSPGEMM_THREADS, 0, s>>>(p->nnz_m, p->mrow, p->colidx_m, p->rowptr_x, p->colidx_x, val_x,
                                                                               p->rowptr_y, p->colidx_y, val_y, out);
    else
        mspgemm_general_kernel<<<entry_grid(p->nnz_m), MSPGEMM_THREADS, 0, s>>>(p->nnz_m, p->mrow, p->colidx_m, p->rowptr_x, p->colidx_x, val_x,
                                                                                p->rowptr_y, p->colidx_y, val_y, out);
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_mspgemm_plan_destroy(void *plan)
{
    delete static_cast<MspgemmPlan *>(plan);
    return SBLAS_OK;
}

} // extern "C"
