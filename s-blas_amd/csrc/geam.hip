// geam.hip -- C = alpha * A + beta * B for two CSR matrices on the device (sblas_hip_geam_plan_*): create does the symbolic
// work once and owns C's rowptr and colidx and the maps dest_a / dest_b, numeric fills C's values for new values of A and
// B and new alpha / beta.  The contract ((S), (V), (I), (D), (M)) stands above the declarations in sblas_hip_geam.h; the
// host restatement is geam_rule.cpp.
//
// The sorted path (every row of A and of B strictly ascending).  Parallel over entries, not rows: a workgroup takes 256
// consecutive entries of one operand, finds the rows of its first and last entry with block_row_of and each thread its
// own row by a binary search between the two, so a row of a million entries is 4000 ordinary workgroups.  With global
// entry indices throughout:
//   mark    per B entry j (row r, column c): lbA[j] = the first A entry of row r with column >= c (a binary search in
//           A's row), u[j] = 1 unless that entry has column c;
//   scan    U = the exclusive scan of u over all of B (radix_sort.h's scan_exclusive; nnz(B) + 1 entries), so that
//           nnz(C) = nnz(A) + U[nnz(B)] and rowptr_C[r] = rowptr_A[r] + U[rowptr_B[r]];
//   place   dest_b[j] = lbA[j] + U[j], matched or not; per A entry i (row r, column c) dest_a[i] = i + U[lbB], lbB the
//           first B entry of row r with column >= c.  colidx_C[dest] is written from both sides (a matched pair writes
//           the same column), and so is src[dest] = (A entry, B entry), -1 for none: the inverse of the maps.
//   numeric one launch over C's entries: fl(fl(alpha * a) + fl(beta * b)) with both sources, the single product with
//           one.  8 B of src, up to 16 B of values read and 8 B written per entry; no LDS, no atomics.
//           Under SBLAS_GEAM_SCATTER instead two launches over the maps: A's terms written through dest_a, then B's
//           through dest_b, added where matched[j] says the first launch left a term (DESIGN.md 3.34 has both timed).
// The general path (any row unsorted or with a duplicate, or SBLAS_GEAM_GENERAL): the plan owns a COO plan
// (SBLAS_COO_SUM) over A's triplets followed by B's -- the rows written by an expansion kernel --, whose rowptr and
// colidx are C's; dest_a / dest_b are read off its perm and runptr; numeric writes [alpha * val_a ; beta * val_b] into
// a buffer of the plan and assembles.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <memory>
#include "../../include/sblas_hip.h"
#include "capi_util.h"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function" // radix_sort.h's sort passes and gathers: the transpose's, not used here
#include "radix_sort.h"
#pragma clang diagnostic pop
#include "geam.h"
#include "rowwise.h" // block_row_of

// alpha * a and t1 + t2 are separate roundings
#pragma clang fp contract(off)

namespace {

using sblas::GEAM_THREADS;
static_assert(GEAM_THREADS == T_THREADS, "the entry passes and the scan share one workgroup size");

// rowptr[0] == 0 and no step down: flag |= 1
__global__ __launch_bounds__(GEAM_THREADS) void geam_rowptr_check_kernel(int64_t rows, const int32_t *__restrict__ rowptr, int *__restrict__ flag)
{
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * GEAM_THREADS + threadIdx.x; i < rows; i += (int64_t)gridDim.x * GEAM_THREADS) {
        if (rowptr[i + 1] < rowptr[i]) bad = 1;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && rowptr[0] != 0) bad = 1;
    if (bad) atomicOr(flag, 1);
}

// a column outside [0, cols): flag |= 1
__global__ __launch_bounds__(GEAM_THREADS) void geam_colidx_check_kernel(int64_t nnz, int64_t cols, const int32_t *__restrict__ colidx,
                                                                         int *__restrict__ flag)
{
    int bad = 0;
    for (int64_t p = (int64_t)blockIdx.x * GEAM_THREADS + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * GEAM_THREADS) {
        const int32_t c = colidx[p];
        if (c < 0 || (int64_t)c >= cols) bad = 1;
    }
    if (bad) atomicOr(flag, 1);
}

// The row of entry e = blockIdx.x * 256 + threadIdx.x of a checked structure (rows >= 1, nnz >= 1); -1 for e >= nnz.
// Every thread of the workgroup must call it: the two block-wide searches bound each thread's own.
__device__ __forceinline__ int entry_row(const int32_t *__restrict__ rowptr, int rows, int nnz, int64_t e)
{
    const int64_t e0 = (int64_t)blockIdx.x * GEAM_THREADS;
    const int64_t e1 = e0 + GEAM_THREADS - 1 < nnz - 1 ? e0 + GEAM_THREADS - 1 : nnz - 1;
    int lo = sblas::block_row_of<GEAM_THREADS>(rowptr, rows, (int)e0);
    int hi = sblas::block_row_of<GEAM_THREADS>(rowptr, rows, (int)e1);
    if (e >= nnz) return -1;
    while (lo < hi) { // the largest r in [lo, hi] with rowptr[r] <= e
        const int mid = (int)(((int64_t)lo + hi + 1) >> 1);
        if (rowptr[mid] <= (int32_t)e) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the first entry in [p0, p1) of an ascending row whose column is >= c; p1 when there is none
__device__ __forceinline__ int32_t lower_bound_col(const int32_t *__restrict__ colidx, int32_t p0, int32_t p1, int32_t c)
{
    while (p0 < p1) {
        const int32_t mid = p0 + ((p1 - p0) >> 1);
        if (colidx[mid] < c) p0 = mid + 1;
        else p1 = mid;
    }
    return p0;
}

// an entry that does not lie strictly above its predecessor in the same row: flag |= 1.  One workgroup per 256 entries.
__global__ __launch_bounds__(GEAM_THREADS) void geam_ascending_kernel(int rows, int nnz, const int32_t *__restrict__ rowptr,
                                                                      const int32_t *__restrict__ colidx, int *__restrict__ flag)
{
    const int64_t e = (int64_t)blockIdx.x * GEAM_THREADS + threadIdx.x;
    const int r = entry_row(rowptr, rows, nnz, e);
    if (r < 0) return;
    if (e > rowptr[r] && colidx[e] <= colidx[e - 1]) atomicOr(flag, 1);
}

// the sorted path, B's side, before the scan: lb[j] and u[j]; u[nnz_b] = 0.  One workgroup per 256 entries of B.
__global__ __launch_bounds__(GEAM_THREADS) void geam_mark_b_kernel(int rows, int nnz_b, const int32_t *__restrict__ rowptr_b,
                                                                   const int32_t *__restrict__ colidx_b, const int32_t *__restrict__ rowptr_a,
                                                                   const int32_t *__restrict__ colidx_a, int32_t *__restrict__ lb,
                                                                   uint32_t *__restrict__ u)
{
    const int64_t j = (int64_t)blockIdx.x * GEAM_THREADS + threadIdx.x;
    const int r = entry_row(rowptr_b, rows, nnz_b, j);
    if (j == 0) u[nnz_b] = 0u;
    if (r < 0) return;
    const int32_t c = colidx_b[j], a1 = rowptr_a[r + 1];
    const int32_t p = lower_bound_col(colidx_a, rowptr_a[r], a1, c);
    lb[j] = p;
    u[j] = (p < a1 && colidx_a[p] == c) ? 0u : 1u;
}

// B's side after the scan: dest_b[j] = lb[j] + U[j] (dest_b holds lb on entry), C's column and the B half of src
__global__ __launch_bounds__(GEAM_THREADS) void geam_place_b_kernel(int64_t nnz_b, const int32_t *__restrict__ colidx_b,
                                                                    const uint32_t *__restrict__ U, int32_t *__restrict__ dest_b,
                                                                    int32_t *__restrict__ colidx_c, int32_t *__restrict__ src,
                                                                    uint8_t *__restrict__ matched)
{
    for (int64_t j = (int64_t)blockIdx.x * GEAM_THREADS + threadIdx.x; j < nnz_b; j += (int64_t)gridDim.x * GEAM_THREADS) {
        const int64_t d = (int64_t)dest_b[j] + U[j]; // < nnz(C) < 2^31: create has checked the total
        dest_b[j] = (int32_t)d;
        if (matched) matched[j] = U[j + 1] == U[j] ? 1 : 0; // u[j] == 0: an A entry has this column
        colidx_c[d] = colidx_b[j];
        src[2 * d + 1] = (int32_t)j;
    }
}

// A's side: dest_a[i] = i + U[lbB], C's column and the A half of src.  One workgroup per 256 entries of A.
__global__ __launch_bounds__(GEAM_THREADS) void geam_place_a_kernel(int rows, int nnz_a, const int32_t *__restrict__ rowptr_a,
                                                                    const int32_t *__restrict__ colidx_a, const int32_t *__restrict__ rowptr_b,
                                                                    const int32_t *__restrict__ colidx_b, const uint32_t *__restrict__ U,
                                                                    int32_t *__restrict__ dest_a, int32_t *__restrict__ colidx_c,
                                                                    int32_t *__restrict__ src)
{
    const int64_t i = (int64_t)blockIdx.x * GEAM_THREADS + threadIdx.x;
    const int r = entry_row(rowptr_a, rows, nnz_a, i);
    if (r < 0) return;
    const int32_t c = colidx_a[i];
    const int32_t p = lower_bound_col(colidx_b, rowptr_b[r], rowptr_b[r + 1], c); // <= nnz(B): U has that entry
    const int64_t d = i + (int64_t)U[p];
    dest_a[i] = (int32_t)d;
    colidx_c[d] = c;
    src[2 * d] = (int32_t)i;
}

// rowptr_c[r] = rowptr_a[r] + U[rowptr_b[r]], r = 0 .. rows
__global__ __launch_bounds__(GEAM_THREADS) void geam_rowptr_kernel(int64_t rows, const int32_t *__restrict__ rowptr_a,
                                                                   const int32_t *__restrict__ rowptr_b, const uint32_t *__restrict__ U,
                                                                   int32_t *__restrict__ rowptr_c)
{
    for (int64_t r = (int64_t)blockIdx.x * GEAM_THREADS + threadIdx.x; r <= rows; r += (int64_t)gridDim.x * GEAM_THREADS)
        rowptr_c[r] = (int32_t)((int64_t)rowptr_a[r] + U[rowptr_b[r]]);
}

// the sorted path's numeric: A's term first, B's added to it; a single term is the product itself
__global__ __launch_bounds__(GEAM_THREADS) void geam_numeric_kernel(int64_t nnz_c, const int2 *__restrict__ src, const double *__restrict__ val_a,
                                                                    const double *__restrict__ val_b, double alpha, double beta,
                                                                    double *__restrict__ val_c)
{
    for (int64_t e = (int64_t)blockIdx.x * GEAM_THREADS + threadIdx.x; e < nnz_c; e += (int64_t)gridDim.x * GEAM_THREADS) {
        const int2 s = src[e];
        double t;
        if (s.x >= 0) {
            t = alpha * val_a[s.x];
            if (s.y >= 0) t = t + beta * val_b[s.y];
        } else {
            t = beta * val_b[s.y];
        }
        val_c[e] = t;
    }
}

// the ordered scatter, first launch: A's terms, each the first on its entry
__global__ __launch_bounds__(GEAM_THREADS) void geam_scatter_a_kernel(int64_t nnz_a, const int32_t *__restrict__ dest_a,
                                                                      const double *__restrict__ val_a, double alpha, double *__restrict__ val_c)
{
    for (int64_t i = (int64_t)blockIdx.x * GEAM_THREADS + threadIdx.x; i < nnz_a; i += (int64_t)gridDim.x * GEAM_THREADS)
        val_c[dest_a[i]] = alpha * val_a[i];
}

// the ordered scatter, second launch: B's terms, added to A's where one matched (the first launch has written it)
__global__ __launch_bounds__(GEAM_THREADS) void geam_scatter_b_kernel(int64_t nnz_b, const int32_t *__restrict__ dest_b,
                                                                      const uint8_t *__restrict__ matched, const double *__restrict__ val_b,
                                                                      double beta, double *val_c)
{
    for (int64_t j = (int64_t)blockIdx.x * GEAM_THREADS + threadIdx.x; j < nnz_b; j += (int64_t)gridDim.x * GEAM_THREADS) {
        const int32_t d = dest_b[j];
        const double t = beta * val_b[j];
        val_c[d] = matched[j] ? val_c[d] + t : t;
    }
}

// the general path: row[off + e] = the row of entry e.  One workgroup per 256 entries.
__global__ __launch_bounds__(GEAM_THREADS) void geam_expand_rows_kernel(int rows, int nnz, const int32_t *__restrict__ rowptr,
                                                                        int32_t *__restrict__ row)
{
    const int64_t e = (int64_t)blockIdx.x * GEAM_THREADS + threadIdx.x;
    const int r = entry_row(rowptr, rows, nnz, e);
    if (r >= 0) row[e] = r;
}

// the general path's maps: the triplets of entry e's run, perm[k] for k in [runptr[e], runptr[e + 1]), land on e
__global__ __launch_bounds__(GEAM_THREADS) void geam_maps_kernel(int64_t nnz_c, int64_t nnz_a, const int32_t *__restrict__ runptr,
                                                                 const int32_t *__restrict__ perm, int32_t *__restrict__ dest_a,
                                                                 int32_t *__restrict__ dest_b)
{
    for (int64_t e = (int64_t)blockIdx.x * GEAM_THREADS + threadIdx.x; e < nnz_c; e += (int64_t)gridDim.x * GEAM_THREADS) {
        for (int32_t k = runptr[e], k1 = runptr[e + 1]; k < k1; ++k) {
            const int64_t t = perm[k];
            if (t < nnz_a) dest_a[t] = (int32_t)e;
            else dest_b[t - nnz_a] = (int32_t)e;
        }
    }
}

// the general path's numeric, first launch: out = [alpha * val_a ; beta * val_b]
__global__ __launch_bounds__(GEAM_THREADS) void geam_scale_kernel(int64_t nnz_a, int64_t nnz_b, const double *__restrict__ val_a,
                                                                  const double *__restrict__ val_b, double alpha, double beta,
                                                                  double *__restrict__ out)
{
    for (int64_t t = (int64_t)blockIdx.x * GEAM_THREADS + threadIdx.x; t < nnz_a + nnz_b; t += (int64_t)gridDim.x * GEAM_THREADS)
        out[t] = t < nnz_a ? alpha * val_a[t] : beta * val_b[t - nnz_a];
}

struct GeamPlan {
    int dev = -1, flags = 0, path = SBLAS_GEAM_PATH_SORTED;
    int64_t rows = 0, cols = 0, nnz_a = 0, nnz_b = 0, nnz_c = 0, a_ascending = 0, b_ascending = 0;
    size_t bytes = 0;
    DeviceBuffer maps, structure, scaled_buf, matched_buf; // dest_a | dest_b; rowptr_c | colidx_c | src (sorted); the scaled values (general)
    int32_t *dest_a = nullptr, *dest_b = nullptr;
    const int32_t *rowptr_c = nullptr, *colidx_c = nullptr;
    int2 *src = nullptr;
    uint8_t *matched = nullptr; // SBLAS_GEAM_SCATTER on the sorted path: B's entry j met an A entry
    double *scaled = nullptr;
    void *coo = nullptr;
    ~GeamPlan()
    {
        if (coo) (void)sblas_hip_coo_plan_destroy(coo);
    }
};

// one workgroup per 256 entries, all of them present: entry_row's searches are block-wide
inline unsigned entry_grid(int64_t nnz) { return (unsigned)ceil_div(nnz, GEAM_THREADS); }

// rowptr (rows + 1 entries) starts at 0 and never steps down; *nnz = rowptr[rows]
hipError_t check_rowptr(hipStream_t s, int64_t rows, const int32_t *rowptr, int *flag, int *bad, int32_t *nnz)
{
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), s);
    if (e != hipSuccess) return e;
    geam_rowptr_check_kernel<<<grid_for(rows), GEAM_THREADS, 0, s>>>(rows, rowptr, flag);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(bad, flag, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(nnz, rowptr + rows, sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
}

hipError_t check_colidx(hipStream_t s, int64_t nnz, int64_t cols, const int32_t *colidx, int *flag, int *bad)
{
    *bad = 0;
    if (nnz == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), s);
    if (e != hipSuccess) return e;
    geam_colidx_check_kernel<<<grid_for(nnz), GEAM_THREADS, 0, s>>>(nnz, cols, colidx, flag);
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
    geam_ascending_kernel<<<entry_grid(nnz), GEAM_THREADS, 0, s>>>((int)rows, (int)nnz, rowptr, colidx, flag);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    *ascending = bad ? 0 : 1;
    return e;
}

// the sorted path's symbolic work; SBLAS_* codes
int create_sorted(GeamPlan &p, hipStream_t s, const int32_t *rowptr_a, const int32_t *colidx_a, const int32_t *rowptr_b, const int32_t *colidx_b)
{
    const int64_t rows = p.rows, na = p.nnz_a, nb = p.nnz_b;
    const size_t da = align16((size_t)na * 4 + 4), db = align16((size_t)nb * 4 + 4);
    if (p.maps.alloc(p.dev, da + db) != hipSuccess) return SBLAS_E_HIP;
    p.dest_a = p.maps.at<int32_t>(), p.dest_b = p.maps.at<int32_t>(da);
    p.bytes += da + db;
    // U and the scan's block sums live until the structure stands
    const int64_t scan_blocks = ceil_div(nb + 1, SCAN_TILE);
    const size_t ub = align16(((size_t)nb + 1) * 4);
    DeviceBuffer scan;
    if (scan.alloc(p.dev, ub + align16((size_t)scan_blocks * 4)) != hipSuccess) return SBLAS_E_HIP;
    uint32_t *U = scan.at<uint32_t>(), *bsum = scan.at<uint32_t>(ub);
    hipError_t e = hipSuccess;
    uint32_t unmatched = 0;
    if (nb > 0) {
        geam_mark_b_kernel<<<entry_grid(nb), GEAM_THREADS, 0, s>>>((int)rows, (int)nb, rowptr_b, colidx_b, rowptr_a, colidx_a, p.dest_b, U);
        e = hipGetLastError();
        if (e == hipSuccess) e = scan_exclusive(s, U, nb + 1, bsum, scan_blocks);
        if (e == hipSuccess) e = hipMemcpyAsync(&unmatched, U + nb, 4, hipMemcpyDeviceToHost, s);
    } else {
        e = hipMemsetAsync(U, 0, 4, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return SBLAS_E_HIP;
    if (sblas_geam_check_nnz(na + (int64_t)unmatched) != SBLAS_OK) return SBLAS_E_INVALID;
    p.nnz_c = na + (int64_t)unmatched;
    const int64_t nc = p.nnz_c;
    const size_t rc = align16(((size_t)rows + 1) * 4), cc = align16((size_t)nc * 4 + 4), sc = align16((size_t)nc * 8 + 8);
    if (p.structure.alloc(p.dev, rc + cc + sc) != hipSuccess) return SBLAS_E_HIP;
    int32_t *rowptr_c = p.structure.at<int32_t>(), *colidx_c = p.structure.at<int32_t>(rc);
    p.src = p.structure.at<int2>(rc + cc); // rc and cc are multiples of 16: the pairs are 8-byte aligned
    p.rowptr_c = rowptr_c, p.colidx_c = colidx_c;
    p.bytes += rc + cc + sc;
    int32_t *src = reinterpret_cast<int32_t *>(p.src);
    if (p.flags == SBLAS_GEAM_SCATTER) {
        if (p.matched_buf.alloc(p.dev, align16((size_t)nb + 1)) != hipSuccess) return SBLAS_E_HIP;
        p.matched = p.matched_buf.at<uint8_t>();
        p.bytes += align16((size_t)nb + 1);
    }
    if (nc > 0) e = hipMemsetAsync(src, 0xff, (size_t)nc * 8, s); // -1: no source
    if (e == hipSuccess && nb > 0) {
        geam_place_b_kernel<<<grid_for(nb), GEAM_THREADS, 0, s>>>(nb, colidx_b, U, p.dest_b, colidx_c, src, p.matched);
        e = hipGetLastError();
    }
    if (e == hipSuccess && na > 0) {
        geam_place_a_kernel<<<entry_grid(na), GEAM_THREADS, 0, s>>>((int)rows, (int)na, rowptr_a, colidx_a, rowptr_b, colidx_b, U, p.dest_a,
                                                                   colidx_c, src);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        geam_rowptr_kernel<<<grid_for(rows + 1), GEAM_THREADS, 0, s>>>(rows, rowptr_a, rowptr_b, U, rowptr_c);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s); // U is freed here
    else (void)hipStreamSynchronize(s);               // and here: no launch is in flight when it goes
    return e == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

// the general path's: the COO plan over A's triplets followed by B's, and the maps off its perm and runptr
int create_general(GeamPlan &p, hipStream_t s, const int32_t *rowptr_a, const int32_t *colidx_a, const int32_t *rowptr_b, const int32_t *colidx_b)
{
    const int64_t rows = p.rows, na = p.nnz_a, nb = p.nnz_b, total = na + nb;
    if (total > INT_MAX) return SBLAS_E_INVALID; // the triplets are sorted in one piece, with int32 positions
    hipError_t e = hipSuccess;
    {
        const size_t tb = align16((size_t)total * 4 + 4);
        DeviceBuffer trip; // row | col of the triplets: the COO plan keeps its own sorted arrays
        if (trip.alloc(p.dev, 2 * tb) != hipSuccess) return SBLAS_E_HIP;
        int32_t *row = trip.at<int32_t>(), *col = trip.at<int32_t>(tb);
        if (na > 0) {
            geam_expand_rows_kernel<<<entry_grid(na), GEAM_THREADS, 0, s>>>((int)rows, (int)na, rowptr_a, row);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(col, colidx_a, (size_t)na * 4, hipMemcpyDeviceToDevice, s);
        }
        if (e == hipSuccess && nb > 0) {
            geam_expand_rows_kernel<<<entry_grid(nb), GEAM_THREADS, 0, s>>>((int)rows, (int)nb, rowptr_b, row + na);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(col + na, colidx_b, (size_t)nb * 4, hipMemcpyDeviceToDevice, s);
        }
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(s); // no launch is in flight when the triplets go
            return SBLAS_E_HIP;
        }
        const int rc = sblas_hip_coo_plan_create(p.dev, s, rows, p.cols, total, total ? row : nullptr, total ? col : nullptr, SBLAS_COO_SUM, &p.coo);
        if (rc != SBLAS_OK) return rc; // create has synchronised: the triplets may go
    }
    int64_t info[8];
    const int32_t *perm = nullptr, *runptr = nullptr;
    if (sblas_hip_coo_plan_info(p.coo, info) != SBLAS_OK || sblas_hip_coo_plan_csr(p.coo, &p.rowptr_c, &p.colidx_c, &perm, &runptr) != SBLAS_OK)
        return SBLAS_E_INVALID;
    p.nnz_c = info[3], p.bytes += (size_t)info[6];
    const size_t da = align16((size_t)na * 4 + 4), db = align16((size_t)nb * 4 + 4), vb = align16((size_t)total * 8 + 8);
    if (p.maps.alloc(p.dev, da + db) != hipSuccess || p.scaled_buf.alloc(p.dev, vb) != hipSuccess) return SBLAS_E_HIP;
    p.dest_a = p.maps.at<int32_t>(), p.dest_b = p.maps.at<int32_t>(da), p.scaled = p.scaled_buf.at<double>();
    p.bytes += da + db + vb;
    if (p.nnz_c > 0) {
        geam_maps_kernel<<<grid_for(p.nnz_c), GEAM_THREADS, 0, s>>>(p.nnz_c, na, runptr, perm, p.dest_a, p.dest_b);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    return e == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

// [a, a + na) and [b, b + nb) doubles share an address
inline bool extents_overlap(const double *a, int64_t na, const double *b, int64_t nb)
{
    if (!a || !b || na <= 0 || nb <= 0) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)nb * 8 && b0 < a0 + (uintptr_t)na * 8;
}

} // namespace

extern "C" {

int sblas_hip_geam_plan_create(int dev, void *stream, int64_t rows, int64_t cols, const int32_t *rowptr_a, const int32_t *colidx_a,
                               const int32_t *rowptr_b, const int32_t *colidx_b, int flags, void **plan_out)
{
    if (!plan_out) return SBLAS_E_INVALID;
    *plan_out = nullptr;
    if (rows < 0 || cols < 0 || rows > INT_MAX - 64 || cols > INT_MAX) return SBLAS_E_INVALID;
    if (flags != SBLAS_GEAM_AUTO && flags != SBLAS_GEAM_GENERAL && flags != SBLAS_GEAM_SCATTER) return SBLAS_E_INVALID;
    if (!rowptr_a || !rowptr_b) return SBLAS_E_INVALID;
    std::unique_ptr<GeamPlan> p(new GeamPlan);
    p->dev = resolve_device(dev), p->flags = flags, p->rows = rows, p->cols = cols;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    hipStream_t s = (hipStream_t)stream;

    // the checks: nothing follows an index before it is known to be in range
    DeviceBuffer small; // a flag
    if (small.alloc(p->dev, 16) != hipSuccess) return SBLAS_E_HIP;
    int *flag = small.at<int>();
    int bad = 0;
    int32_t nnz_a = 0, nnz_b = 0;
    if (check_rowptr(s, rows, rowptr_a, flag, &bad, &nnz_a) != hipSuccess) return SBLAS_E_HIP;
    if (bad) return SBLAS_E_INVALID;
    if (check_rowptr(s, rows, rowptr_b, flag, &bad, &nnz_b) != hipSuccess) return SBLAS_E_HIP;
    if (bad) return SBLAS_E_INVALID;
    if ((nnz_a > 0 && !colidx_a) || (nnz_b > 0 && !colidx_b)) return SBLAS_E_INVALID;
    if (check_colidx(s, nnz_a, cols, colidx_a, flag, &bad) != hipSuccess) return SBLAS_E_HIP;
    if (bad) return SBLAS_E_INVALID;
    if (check_colidx(s, nnz_b, cols, colidx_b, flag, &bad) != hipSuccess) return SBLAS_E_HIP;
    if (bad) return SBLAS_E_INVALID;
    p->nnz_a = nnz_a, p->nnz_b = nnz_b;

    // one pass over each colidx: strictly ascending rows or not
    if (check_ascending(s, rows, nnz_a, rowptr_a, colidx_a, flag, &p->a_ascending) != hipSuccess) return SBLAS_E_HIP;
    if (check_ascending(s, rows, nnz_b, rowptr_b, colidx_b, flag, &p->b_ascending) != hipSuccess) return SBLAS_E_HIP;
    p->path = (flags != SBLAS_GEAM_GENERAL && p->a_ascending && p->b_ascending) ? SBLAS_GEAM_PATH_SORTED : SBLAS_GEAM_PATH_GENERAL;
    const int rc = p->path == SBLAS_GEAM_PATH_SORTED ? create_sorted(*p, s, rowptr_a, colidx_a, rowptr_b, colidx_b)
                                                     : create_general(*p, s, rowptr_a, colidx_a, rowptr_b, colidx_b);
    if (rc != SBLAS_OK) return rc;
    *plan_out = p.release();
    return SBLAS_OK;
}

int sblas_hip_geam_plan_info(const void *plan, int64_t out[12])
{
    if (!plan || !out) return SBLAS_E_INVALID;
    const GeamPlan *p = static_cast<const GeamPlan *>(plan);
    out[0] = p->rows, out[1] = p->cols, out[2] = p->nnz_a, out[3] = p->nnz_b, out[4] = p->nnz_c, out[5] = p->nnz_a + p->nnz_b - p->nnz_c;
    out[6] = p->path, out[7] = p->a_ascending, out[8] = p->b_ascending;
    out[9] = p->nnz_c == 0 ? 0 : p->path == SBLAS_GEAM_PATH_SORTED && !p->matched ? sblas::GEAM_SORTED_LAUNCHES : sblas::GEAM_GENERAL_LAUNCHES;
    out[10] = (int64_t)p->bytes, out[11] = p->flags;
    return SBLAS_OK;
}

int sblas_hip_geam_plan_csr(const void *plan, const int32_t **rowptr_c, const int32_t **colidx_c)
{
    if (!plan) return SBLAS_E_INVALID;
    const GeamPlan *p = static_cast<const GeamPlan *>(plan);
    if (rowptr_c) *rowptr_c = p->rowptr_c;
    if (colidx_c) *colidx_c = p->colidx_c;
    return SBLAS_OK;
}

int sblas_hip_geam_plan_maps(const void *plan, const int32_t **dest_a, const int32_t **dest_b)
{
    if (!plan) return SBLAS_E_INVALID;
    const GeamPlan *p = static_cast<const GeamPlan *>(plan);
    if (dest_a) *dest_a = p->dest_a;
    if (dest_b) *dest_b = p->dest_b;
    return SBLAS_OK;
}

int sblas_hip_geam_plan_numeric(const void *plan, void *stream, const double *val_a, const double *val_b, double alpha, double beta,
                                double *val_c)
{
    if (!plan) return SBLAS_E_INVALID;
    const GeamPlan *p = static_cast<const GeamPlan *>(plan);
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID; // the plan's arrays live on its own device
    if (p->nnz_c == 0) return SBLAS_OK;
    if (!val_c || (p->nnz_a > 0 && !val_a) || (p->nnz_b > 0 && !val_b)) return SBLAS_E_INVALID;
    if (extents_overlap(val_c, p->nnz_c, val_a, p->nnz_a) || extents_overlap(val_c, p->nnz_c, val_b, p->nnz_b)) return SBLAS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (p->path == SBLAS_GEAM_PATH_SORTED && p->matched) { // every entry of C has a term: A's first, then B's
        if (p->nnz_a > 0) geam_scatter_a_kernel<<<grid_for(p->nnz_a), GEAM_THREADS, 0, s>>>(p->nnz_a, p->dest_a, val_a, alpha, val_c);
        if (p->nnz_b > 0) geam_scatter_b_kernel<<<grid_for(p->nnz_b), GEAM_THREADS, 0, s>>>(p->nnz_b, p->dest_b, p->matched, val_b, beta, val_c);
        return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
    }
    if (p->path == SBLAS_GEAM_PATH_SORTED) {
        geam_numeric_kernel<<<grid_for(p->nnz_c), GEAM_THREADS, 0, s>>>(p->nnz_c, p->src, val_a, val_b, alpha, beta, val_c);
        return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
    }
    geam_scale_kernel<<<grid_for(p->nnz_a + p->nnz_b), GEAM_THREADS, 0, s>>>(p->nnz_a, p->nnz_b, val_a, val_b, alpha, beta, p->scaled);
    if (hipGetLastError() != hipSuccess) return SBLAS_E_HIP;
    return sblas_hip_coo_plan_assemble(p->coo, s, p->scaled, val_c);
}

int sblas_hip_geam_plan_destroy(void *plan)
{
    delete static_cast<GeamPlan *>(plan);
    return SBLAS_OK;
}

} // extern "C"
