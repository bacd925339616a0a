// sddmm_narrow.hip -- the narrow SDDMM for gfx950 (wave64): out[e] = alpha * <X[row(e), :k], Y[col(e), :k]> + beta * out[e]
// for k <= 8 on a part of a CSR pattern, and its C-ABI entry (include/sblas_hip_sddmm_narrow.h).  DESIGN.md 3.38.
//
//   sddmm_narrow_kernel<K, VEC>   a workgroup per run of SDDMM_NARROW_CHUNK consecutive nonzeros, four per lane
//
// Parallel over nonzeros, as sddmm_kernel is: a workgroup finds the rows of its first and last nonzero by a 256-way search
// in rowptr, marks the row starts that fall inside its run in LDS and turns them into row indices with a max-scan.  The
// scan hands lane t the rows of the entries 4t .. 4t + 3 in four registers, and those are the entries the lane owns: the
// row indices never go back to LDS.  A lane reads its four column indices in one 16-byte load, issues the gathers of all
// its rows of Y and of the rows of X it needs -- one per change of the row index, the others are register copies -- before
// the first fma, and writes its four results with two 16-byte stores.  No result array in LDS, no lane exchange after the
// scan, no atomics on global memory, no scratch.  The order of a sum is sddmm_narrow_dot's (sddmm_narrow.h), which is
// sddmm_kernel's at k <= 8: neither the place of an entry nor an alignment enters it.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include "../../include/sblas_hip.h"
#include "capi_util.h"
#include "kernels.h"
#include "rowwise.h" // block_row_of
#include "sddmm_narrow.h"

namespace sblas {

// the first K elements of a row into r[0 .. K), the padding behind them is left as it is (+0)
template <int K, bool VEC> __device__ __forceinline__ void narrow_load_row(const double *__restrict__ row, double *r)
{
    if constexpr (VEC) {
#pragma unroll
        for (int j = 0; j + 1 < K; j += 2) {
            const double2 v = *reinterpret_cast<const double2 *>(row + j);
            r[j] = v.x, r[j + 1] = v.y;
        }
        if constexpr (K % 2 == 1) r[K - 1] = row[K - 1];
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j) r[j] = row[j];
    }
}

// flags: bit 0, colidx is 16-byte aligned; bit 1, out is.  (A run starts a multiple of 1024 entries into both.)
constexpr int NARROW_COLIDX16 = 1, NARROW_OUT16 = 2;

template <int K, bool VEC>
__global__ __launch_bounds__(SDDMM_NARROW_THREADS) void sddmm_narrow_kernel(int rows, int nnz, int nchunks, const int *__restrict__ rowptr,
                                                                             const int *__restrict__ colidx, const double *__restrict__ X,
                                                                             int64_t ldx, const double *__restrict__ Y, int64_t ldy,
                                                                             double alpha, double beta, int part, int flags,
                                                                             double *__restrict__ out)
{
    constexpr int THREADS = SDDMM_NARROW_THREADS, CHUNK = SDDMM_NARROW_CHUNK, EPL = SDDMM_NARROW_EPL;
    constexpr int KP = sddmm_narrow_padded(K);
    static_assert(EPL == 4 && CHUNK == 4 * THREADS, "a lane's entries are the int4 of its scan");
    __shared__ int rowof[CHUNK];
    __shared__ int wave_max[THREADS / 64];
    const int tid = threadIdx.x;
    const int chunk = xcd_contiguous_panel((int)blockIdx.x, nchunks);
    const int e0 = chunk * CHUNK;
    const int cnt = min(CHUNK, nnz - e0);

    // ---- one row index per nonzero of the run, four in the registers of the lane that owns them ----
    const int r_lo = block_row_of<THREADS>(rowptr, rows, e0);
    const int r_hi = block_row_of<THREADS>(rowptr, rows, e0 + cnt - 1);
    reinterpret_cast<int4 *>(rowof)[tid] = make_int4(r_lo, r_lo, r_lo, r_lo);
    __syncthreads();
    for (int64_t r = (int64_t)r_lo + 1 + tid; r <= r_hi; r += THREADS) {
        const int s = rowptr[r] - e0; // in (0, cnt): r_lo is the last row that starts at or before e0
        if (s > 0 && s < cnt) atomicMax(&rowof[s], (int)r); // rows that start together: the last one owns the entry
    }
    __syncthreads();
    int row[EPL];
    {
        int4 v = reinterpret_cast<int4 *>(rowof)[tid];
        v.y = max(v.y, v.x), v.z = max(v.z, v.y), v.w = max(v.w, v.z);
        int m = v.w;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(m, o);
            if ((tid & 63) >= o) m = max(m, u);
        }
        if ((tid & 63) == 63) wave_max[tid >> 6] = m;
        __syncthreads();
        int before = __shfl_up(m, 1);
        if ((tid & 63) == 0) before = r_lo;
        for (int w = 0; w < (tid >> 6); ++w) before = max(before, wave_max[w]);
        row[0] = max(v.x, before), row[1] = max(v.y, before), row[2] = max(v.z, before), row[3] = max(v.w, before);
    }

    // ---- the lane's entries [i0, i0 + n) of the run: n is 4 except in the last lanes of the last run ----
    const int i0 = EPL * tid;
    const int n = min(EPL, cnt - i0); // may be <= 0
    const int *cp = colidx + e0 + i0;
    int col[EPL] = {0, 0, 0, 0};
    if (n == EPL && (flags & NARROW_COLIDX16)) {
        const int4 cv = *reinterpret_cast<const int4 *>(cp);
        col[0] = cv.x, col[1] = cv.y, col[2] = cv.z, col[3] = cv.w;
    } else {
#pragma unroll
        for (int j = 0; j < EPL; ++j)
            if (j < n) col[j] = cp[j];
    }
    bool inside[EPL], own[EPL]; // own: the entry loads its row of X; otherwise it has the row of the entry before it
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        inside[j] = j < n && sddmm_narrow_in_part(part, row[j], col[j]);
        own[j] = inside[j] && !(j > 0 && inside[j - 1] && row[j] == row[j - 1]);
    }
    // every gather in flight before the first fma; an entry outside the part (or the run) reads nothing
    double x[EPL][KP], y[EPL][KP];
#pragma unroll
    for (int j = 0; j < EPL; ++j)
#pragma unroll
        for (int q = 0; q < KP; ++q) x[j][q] = y[j][q] = 0.0;
#pragma unroll
    for (int j = 0; j < EPL; ++j)
        if (inside[j]) narrow_load_row<K, VEC>(Y + (int64_t)col[j] * ldy, y[j]);
#pragma unroll
    for (int j = 0; j < EPL; ++j)
        if (own[j]) narrow_load_row<K, VEC>(X + (int64_t)row[j] * ldx, x[j]);
    double *op = out + e0 + i0;
    const bool out16 = n == EPL && (flags & NARROW_OUT16);
    double old[EPL] = {0.0, 0.0, 0.0, 0.0};
    if (beta != 0.0) {
        if (out16) {
            const double2 a = reinterpret_cast<const double2 *>(op)[0], b = reinterpret_cast<const double2 *>(op)[1];
            old[0] = a.x, old[1] = a.y, old[2] = b.x, old[3] = b.y;
        } else {
#pragma unroll
            for (int j = 0; j < EPL; ++j)
                if (j < n) old[j] = op[j];
        }
    }
#pragma unroll
    for (int j = 1; j < EPL; ++j)
        if (inside[j] && !own[j]) {
#pragma unroll
            for (int q = 0; q < K; ++q) x[j][q] = x[j - 1][q];
        }
    double res[EPL];
#pragma unroll
    for (int j = 0; j < EPL; ++j) res[j] = sddmm_narrow_out(inside[j], sddmm_narrow_dot(x[j], y[j], KP), alpha, beta, old[j]);
    if (out16) {
        reinterpret_cast<double2 *>(op)[0] = make_double2(res[0], res[1]);
        reinterpret_cast<double2 *>(op)[1] = make_double2(res[2], res[3]);
    } else {
#pragma unroll
        for (int j = 0; j < EPL; ++j)
            if (j < n) op[j] = res[j];
    }
}

template <int K>
static void launch_narrow_k(hipStream_t s, bool vec, int nchunks, int rows, int nnz, const int *rowptr, const int *colidx,
                            const double *X, int64_t ldx, const double *Y, int64_t ldy, double alpha, double beta, int part,
                            int flags, double *out)
{
#define NARROW_K(V)                                                                                                            \
    hipLaunchKernelGGL((sddmm_narrow_kernel<K, V>), dim3(nchunks), dim3(SDDMM_NARROW_THREADS), 0, s, rows, nnz, nchunks, rowptr, \
                       colidx, X, ldx, Y, ldy, alpha, beta, part, flags, out)
    if constexpr (K > 1) { // k = 1: a row is one 8-byte load either way
        if (vec) {
            NARROW_K(true);
            return;
        }
    }
    NARROW_K(false);
#undef NARROW_K
}

static hipError_t launch_sddmm_narrow(hipStream_t s, int rows, int nnz, const int *rowptr, const int *colidx, const double *X,
                                      int64_t ldx, const double *Y, int64_t ldy, int k, double alpha, double beta, int part,
                                      double *out)
{
    const bool vec = aligned16(X) && aligned16(Y) && ldx % 2 == 0 && ldy % 2 == 0;
    const int flags = (aligned16(colidx) ? NARROW_COLIDX16 : 0) | (aligned16(out) ? NARROW_OUT16 : 0);
    const int nchunks = (int)(((int64_t)nnz + SDDMM_NARROW_CHUNK - 1) / SDDMM_NARROW_CHUNK); // nnz may be INT_MAX
#define NARROW_GO(KK) launch_narrow_k<KK>(s, vec, nchunks, rows, nnz, rowptr, colidx, X, ldx, Y, ldy, alpha, beta, part, flags, out)
    switch (k) {
    case 1: NARROW_GO(1); break;
    case 2: NARROW_GO(2); break;
    case 3: NARROW_GO(3); break;
    case 4: NARROW_GO(4); break;
    case 5: NARROW_GO(5); break;
    case 6: NARROW_GO(6); break;
    case 7: NARROW_GO(7); break;
    default: NARROW_GO(8);
    }
#undef NARROW_GO
    return hipGetLastError();
}

} // namespace sblas

extern "C" int sblas_hip_sddmm_narrow_f64_i32(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr,
                                              const int32_t *colidx, const double *X, int64_t ldx, const double *Y, int64_t ldy,
                                              int k, double alpha, double beta, int part, double *out)
{
    if (!csr_args_ok(rows, cols, nnz, rowptr, colidx, out)) return SBLAS_E_INVALID;
    if (k < 1 || k > sblas::SDDMM_NARROW_MAX_K || ldx < k || ldy < k || !sblas::sddmm_narrow_part_ok(part)) return SBLAS_E_INVALID;
    if (nnz == 0) return SBLAS_OK;
    if (rows == 0 || cols == 0 || !X || !Y) return SBLAS_E_INVALID; // entries without a place
    if (sblas::options().validate)
        if (const int vrc = sblas_hip_debug_validate_csr_i32(dev, stream, rows, cols, nnz, rowptr, colidx)) return vrc;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    return sblas::launch_sddmm_narrow((hipStream_t)stream, (int)rows, (int)nnz, rowptr, colidx, X, ldx, Y, ldy, k, alpha, beta,
                                      part, out) == hipSuccess
               ? SBLAS_OK
               : SBLAS_E_HIP;
}
