// softmax.hip -- softmax over the stored entries of each row of a CSR pattern (edge softmax) for gfx950 (wave64), its
// backward, and their C-ABI entry points (include/sblas_hip.h, "Row-wise softmax").  DESIGN.md 3.16.
//
//   forward    t[e] = scale * x[e],  m = max t,  s = sum exp(t[e] - m),  out[e] = exp(t[e] - m) / s        (per row)
//   backward   d = sum p[e] * dp[e],  dx[e] = (scale * p[e]) * (dp[e] - d)                                 (per row)
//
//   softmax_rows_kernel<BWD, TR>   a wave per TR consecutive rows; every row of at most SM_SUPER entries
//   softmax_long_kernel<PHASE>     a workgroup per SM_SUPER consecutive value positions; the rows longer than SM_SUPER
//
// Work split.  Only rowptr is read, never a host copy of it.  The rows kernel gives a wave TR = 8 rows (TR = 2 when rows
// average 64 entries or more): when all eight hold at most 8 entries, 8 lanes take a row each and the wave does them in
// one go; otherwise the wave takes the rows one after the other, a row of up to 512 entries in registers (one read, one
// write), a row of up to SM_SUPER = 4096 in three passes over data its first pass pulled into the cache.  It skips longer
// rows.  Those belong to the long kernels, launched whenever nnz > SM_SUPER, a workgroup per block of 4096 value
// positions: a long row is cut into supercells of 4096 entries counted from the ROW's start, and the workgroup whose
// block holds a supercell's first entry owns it whole (at most two per workgroup: one of the row that runs into the
// block, one of the row that starts in it).  Forward: per-supercell max -> row max, per-supercell sums -> row sum, out;
// backward: per-supercell dot -> row dot, dx.  The per-supercell figures live in the workspace, in slot
// 2 * (first entry / 4096) + (first supercell of its row ? 1 : 0), which no two supercells share.
//
// Summation order (a function of the row's length L alone).  The entries of a row are numbered 0 .. L - 1 in stored
// order.  Leaf i is exp(t[i] - m) (backward: fma(p[i], dp[i], +0)).  A cell is 64 consecutive leaves from a multiple of
// 64, absent ones +0; it is summed by the butterfly v += v[l ^ 1], v += v[l ^ 2], v += v[l ^ 4], v += v[l ^ 8],
// v += v[l ^ 16], v += v[l ^ 32] over its 64 places.  A supercell is 64 consecutive cells from a multiple of 64, absent
// ones +0, summed by the same butterfly over the 64 cell sums.  The row sum is +0 plus the supercell sums, added left to
// right.  (A leaf is never -0, so adding an absent +0 changes nothing: the 8-lane group, the single-cell row and the
// single-supercell row skip the levels that would only add zeros.)  The max is exact in any order; it propagates NaN.
// scale * x, t - m, e / s, scale * p, dp - d and the final product are separate roundings: contraction is off below.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include "../../include/sblas_hip.h"
#include "capi_util.h"
#include "kernels.h"
#include "rowwise.h" // fold_sum, fold_max, nmax, fwd_out, bwd_out, block_row_of, supercell_slot

#pragma clang fp contract(off)

namespace sblas {
namespace {

constexpr int SM_THREADS = 256;
constexpr int SM_WAVES = SM_THREADS / 64;
constexpr int SM_CELL = ROW_CELL;   // leaves per cell: one wave-wide butterfly
constexpr int SM_SUPER = ROW_SUPER; // leaves per supercell: 64 cells; the longest row the rows kernel takes
constexpr int SM_REG_CELLS = 8; // cells of a row a wave keeps in registers
constexpr int SM_GROUP = 8;     // lanes per row when the eight rows of a wave hold at most 8 entries each

// ---- the leaves and the outputs, the same expressions on every path --------------------------------------------------
// forward: a = x; backward: a = p, b = dp
// (fwd_out, bwd_out: rowwise.h)

// One row of at most 64 * NC entries, kept in registers by one wave.  a, b, out are already advanced to the row.
template <bool BWD, int NC>
__device__ __forceinline__ void row_in_registers(int len, int lane, const double *a, const double *b, double scale, double *out)
{
    double v[NC], w[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int i = c * SM_CELL + lane;
        const bool on = i < len;
        if constexpr (BWD) {
            v[c] = on ? a[i] : 0.0;
            w[c] = on ? b[i] : 0.0;
        } else {
            v[c] = on ? scale * a[i] : NEG_INF;
        }
    }
    double m = 0.0;
    if constexpr (!BWD) {
        m = v[0];
#pragma unroll
        for (int c = 1; c < NC; ++c) m = nmax(m, v[c]);
        m = fold_max<64>(m);
    }
    double cs = 0.0, s = 0.0; // lane c holds the sum of cell c
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if (c * SM_CELL < len) {
            const bool on = c * SM_CELL + lane < len;
            double leaf;
            if constexpr (BWD) leaf = fma(v[c], w[c], 0.0); // absent: fma(+0, +0, +0)
            else leaf = v[c] = on ? exp(v[c] - m) : 0.0;
            const double sc = fold_sum<64>(leaf);
            if (NC == 1) s = sc;
            else if (lane == c) cs = sc;
        }
    }
    if (NC > 1) s = fold_sum<64>(cs);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int i = c * SM_CELL + lane;
        if (i < len) out[i] = BWD ? bwd_out(v[c], w[c], s, scale) : v[c] / s;
    }
}

// One row of up to SM_SUPER entries by one wave, in passes (the row stays in the cache between them)
template <bool BWD>
__device__ __forceinline__ void row_in_passes(int len, int lane, const double *a, const double *b, double scale, double *out)
{
    const int ncell = (len + SM_CELL - 1) / SM_CELL; // <= 64
    double m = NEG_INF;
    if constexpr (!BWD) {
        for (int c = 0; c < ncell; ++c) {
            const int i = c * SM_CELL + lane;
            if (i < len) m = nmax(m, scale * a[i]);
        }
        m = fold_max<64>(m);
    }
    double cs = 0.0;
    for (int c = 0; c < ncell; ++c) {
        const int i = c * SM_CELL + lane;
        double leaf = 0.0;
        if (i < len) leaf = BWD ? fma(a[i], b[i], 0.0) : exp(scale * a[i] - m);
        const double sc = fold_sum<64>(leaf);
        if (lane == c) cs = sc;
    }
    const double s = fold_sum<64>(cs);
    for (int c = 0; c < ncell; ++c) {
        const int i = c * SM_CELL + lane;
        if (i < len) out[i] = BWD ? bwd_out(a[i], b[i], s, scale) : fwd_out(scale * a[i], m, s);
    }
}

template <bool BWD>
__device__ __forceinline__ void row_by_wave(int beg, int len, int lane, const double *a, const double *b, double scale, double *out)
{
    if (len <= 0 || len > SM_SUPER) return; // empty: nothing; longer: the long kernels
    a += beg, out += beg;
    if (BWD) b += beg;
    if (len <= SM_CELL) row_in_registers<BWD, 1>(len, lane, a, b, scale, out);
    else if (len <= SM_CELL * SM_REG_CELLS) row_in_registers<BWD, SM_REG_CELLS>(len, lane, a, b, scale, out);
    else row_in_passes<BWD>(len, lane, a, b, scale, out);
}

// a, b, out carry no __restrict__: out may be a (forward) or b (backward); every entry is read and written by one lane
template <bool BWD, int TR>
__global__ __launch_bounds__(SM_THREADS) void softmax_rows_kernel(int rows, const int *__restrict__ rowptr, const double *a,
                                                                  const double *b, double scale, double *out)
{
    const int lane = threadIdx.x & 63;
    const int64_t r0 = ((int64_t)blockIdx.x * SM_WAVES + (threadIdx.x >> 6)) * TR;
    if (r0 >= rows) return;
    // lanes 0 .. TR hold rowptr[r0 .. r0 + TR], rows beyond the last one come out empty
    const int64_t ri = r0 + (lane <= TR ? lane : TR);
    const int rp = rowptr[ri < rows ? ri : rows];
    if constexpr (TR == SM_GROUP) {
        const int g = lane / SM_GROUP, j = lane % SM_GROUP;
        const int beg = __shfl(rp, g, 64), len = __shfl(rp, g + 1, 64) - beg;
        if (__all(len <= SM_GROUP)) {
            const bool on = j < len;
            const int64_t e = (int64_t)beg + j;
            if constexpr (BWD) {
                const double p = on ? a[e] : 0.0, dp = on ? b[e] : 0.0;
                const double d = fold_sum<SM_GROUP>(fma(p, dp, 0.0));
                if (on) out[e] = bwd_out(p, dp, d, scale);
            } else {
                const double t = on ? scale * a[e] : NEG_INF;
                const double m = fold_max<SM_GROUP>(t);
                const double ex = on ? exp(t - m) : 0.0;
                const double s = fold_sum<SM_GROUP>(ex);
                if (on) out[e] = ex / s;
            }
            return;
        }
    }
#pragma unroll
    for (int q = 0; q < TR; ++q) {
        const int beg = __builtin_amdgcn_readlane(rp, q), end = __builtin_amdgcn_readlane(rp, q + 1);
        row_by_wave<BWD>(beg, end - beg, lane, a, b, scale, out);
    }
}

// ---- rows longer than SM_SUPER ----------------------------------------------------------------------------------------
enum { PH_MAX = 0, PH_SUM = 1, PH_OUT = 2, PH_DOT = 3, PH_DX = 4 };

// PHASE: PH_MAX -> pmax[slot]; PH_SUM reads the row's pmax -> psum[slot]; PH_OUT reads both -> out.
//        PH_DOT -> psum[slot]; PH_DX reads the row's psum -> out.
template <int PHASE>
__global__ __launch_bounds__(SM_THREADS) void softmax_long_kernel(int rows, int nnz, const int *__restrict__ rowptr, const double *a,
                                                                  const double *b, double scale, double *out, double *pmax,
                                                                  double *psum)
{
    __shared__ double cell_sum[SM_CELL];
    __shared__ double wave_part[SM_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t e_first = (int64_t)blockIdx.x * SM_SUPER;
    const int64_t e_last = e_first + SM_SUPER - 1 < nnz ? e_first + SM_SUPER - 1 : (int64_t)nnz - 1;
    const int r_a = block_row_of<SM_THREADS>(rowptr, rows, (int)e_first), r_b = block_row_of<SM_THREADS>(rowptr, rows, (int)e_last);
    for (int which = 0; which < 2; ++which) {
        if (which == 1 && r_b == r_a) break;
        const int r = which ? r_b : r_a;
        const int64_t row_beg = rowptr[r], len = (int64_t)rowptr[r + 1] - row_beg;
        if (len <= SM_SUPER) continue;
        const int64_t k = row_beg >= e_first ? 0 : (e_first - row_beg + SM_SUPER - 1) / SM_SUPER;
        const int64_t p = row_beg + k * SM_SUPER; // first entry of the supercell that can start in this block
        if (p > e_last || p >= row_beg + len) continue;
        const int cnt = (int)(row_beg + len - p < SM_SUPER ? row_beg + len - p : SM_SUPER);
        const int ncell = (cnt + SM_CELL - 1) / SM_CELL;
        const int64_t slot = supercell_slot(row_beg, p);
        const int64_t nsuper = (len + SM_SUPER - 1) / SM_SUPER;
        const double *ap = a + p;
        const double *bp = b + p; // backward only
        double *op = out + p;

        if constexpr (PHASE == PH_MAX) {
            double m = NEG_INF;
            for (int i = tid; i < cnt; i += SM_THREADS) m = nmax(m, scale * ap[i]);
            m = fold_max<64>(m);
            __syncthreads(); // wave_part of the previous round has been read
            if (lane == 0) wave_part[wave] = m;
            __syncthreads();
            if (tid == 0) pmax[slot] = nmax(nmax(wave_part[0], wave_part[1]), nmax(wave_part[2], wave_part[3]));
            continue;
        }
        // the row's max, from the maxima of its supercells
        double m = NEG_INF;
        if constexpr (PHASE == PH_SUM || PHASE == PH_OUT) {
            for (int64_t q = tid; q < nsuper; q += SM_THREADS) m = nmax(m, pmax[supercell_slot(row_beg, row_beg + q * SM_SUPER)]);
            m = fold_max<64>(m);
            __syncthreads();
            if (lane == 0) wave_part[wave] = m;
            __syncthreads();
            m = nmax(nmax(wave_part[0], wave_part[1]), nmax(wave_part[2], wave_part[3]));
        }
        if constexpr (PHASE == PH_SUM || PHASE == PH_DOT) {
            __syncthreads(); // cell_sum of the previous round has been read
            if (tid < SM_CELL) cell_sum[tid] = 0.0;
            __syncthreads();
            for (int c = wave; c < ncell; c += SM_WAVES) {
                const int i = c * SM_CELL + lane;
                double leaf = 0.0;
                if (i < cnt) leaf = PHASE == PH_DOT ? fma(ap[i], bp[i], 0.0) : exp(scale * ap[i] - m);
                const double sc = fold_sum<64>(leaf);
                if (lane == 0) cell_sum[c] = sc;
            }
            __syncthreads();
            if (wave == 0) {
                const double s = fold_sum<64>(cell_sum[lane]);
                if (lane == 0) psum[slot] = s;
            }
            continue;
        }
        if constexpr (PHASE == PH_OUT || PHASE == PH_DX) {
            double s = 0.0; // the supercell sums, left to right
            for (int64_t q = 0; q < nsuper; ++q) s += psum[supercell_slot(row_beg, row_beg + q * SM_SUPER)];
            for (int i = tid; i < cnt; i += SM_THREADS)
                op[i] = PHASE == PH_DX ? bwd_out(ap[i], bp[i], s, scale) : fwd_out(scale * ap[i], m, s);
        }
    }
}

// SBLAS_VALIDATE=1: flag |= 1 when a row pointer runs backwards or outside [0, nnz], 2 when the ends are not 0 and nnz
__global__ __launch_bounds__(SM_THREADS) void softmax_validate_kernel(int64_t rows, int64_t nnz, const int *__restrict__ rowptr,
                                                                      int *__restrict__ flag)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int bad = 0;
    for (int64_t r = tid; r < rows; r += stride) {
        const int lo = rowptr[r], hi = rowptr[r + 1];
        if (lo > hi || lo < 0 || (int64_t)hi > nnz) bad |= 1;
    }
    if (tid == 0 && (rowptr[0] != 0 || (int64_t)rowptr[rows] != nnz)) bad |= 2;
    if (bad) atomicOr(flag, bad);
}

hipError_t validate_rowptr(hipStream_t s, int64_t rows, int64_t nnz, const int *rowptr, int *bad)
{
    int *flag = nullptr;
    hipError_t e = hipMalloc(&flag, sizeof(int));
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(flag, 0, sizeof(int), s);
    if (e == hipSuccess) {
        const int64_t blocks = (rows + SM_THREADS - 1) / SM_THREADS;
        hipLaunchKernelGGL(softmax_validate_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(SM_THREADS), 0, s, rows, nnz,
                           rowptr, flag);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(bad, flag, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(flag);
    return e;
}

int64_t softmax_slots(int64_t nnz) { return 2 * ((nnz + SM_SUPER - 1) / SM_SUPER) + 2; }

template <bool BWD>
hipError_t launch_softmax(hipStream_t s, int rows, int nnz, const int *rowptr, const double *a, const double *b, double scale,
                          double *out, void *workspace)
{
    // rows of 64 entries or more on average: two rows a wave (more waves, evener); shorter: eight, for the 8-lane groups
    if ((int64_t)nnz >= (int64_t)rows * SM_CELL) {
        const unsigned grid = (unsigned)(((int64_t)rows + 2 * SM_WAVES - 1) / (2 * SM_WAVES));
        hipLaunchKernelGGL((softmax_rows_kernel<BWD, 2>), dim3(grid), dim3(SM_THREADS), 0, s, rows, rowptr, a, b, scale, out);
    } else {
        const unsigned grid = (unsigned)(((int64_t)rows + SM_GROUP * SM_WAVES - 1) / (SM_GROUP * SM_WAVES));
        hipLaunchKernelGGL((softmax_rows_kernel<BWD, SM_GROUP>), dim3(grid), dim3(SM_THREADS), 0, s, rows, rowptr, a, b, scale, out);
    }
    if (nnz > SM_SUPER) { // a row longer than a supercell is possible
        double *pmax = static_cast<double *>(workspace), *psum = pmax + softmax_slots(nnz);
        const unsigned grid = (unsigned)(((int64_t)nnz + SM_SUPER - 1) / SM_SUPER);
#define SM_LONG(PHASE)                                                                                                         \
    hipLaunchKernelGGL((softmax_long_kernel<PHASE>), dim3(grid), dim3(SM_THREADS), 0, s, rows, nnz, rowptr, a, b, scale, out,   \
                       pmax, psum)
        if (BWD) {
            SM_LONG(PH_DOT);
            SM_LONG(PH_DX);
        } else {
            SM_LONG(PH_MAX);
            SM_LONG(PH_SUM);
            SM_LONG(PH_OUT);
        }
#undef SM_LONG
    }
    return hipGetLastError();
}

// the checks both entry points share; SBLAS_OK with *go = false: nothing to do
int softmax_args(int dev, void *stream, int64_t rows, int64_t nnz, const int32_t *rowptr, const void *in0, const void *in1,
                 const void *out, void *workspace, size_t workspace_bytes, bool *go)
{
    *go = false;
    if (rows < 0 || nnz < 0 || rows > INT_MAX - 64 || nnz > INT_MAX || !rowptr) return SBLAS_E_INVALID;
    if (nnz > 0 && (!in0 || !in1 || !out)) return SBLAS_E_INVALID;
    if (nnz == 0) return SBLAS_OK;
    if (rows == 0) return SBLAS_E_INVALID; // entries without a row
    const size_t need = sblas_hip_csr_softmax_workspace(rows, nnz);
    if (need > 0 && (!workspace || workspace_bytes < need)) return SBLAS_E_WORKSPACE;
    if (need > 0 && !aligned16(workspace)) return SBLAS_E_INVALID;
    if (sblas::options().validate) {
        DeviceScope scope(dev);
        if (scope.err != hipSuccess) return SBLAS_E_HIP;
        int bad = 0;
        if (validate_rowptr((hipStream_t)stream, rows, nnz, rowptr, &bad) != hipSuccess) return SBLAS_E_HIP;
        if (bad) return SBLAS_E_INVALID;
    }
    *go = true;
    return SBLAS_OK;
}

} // namespace
} // namespace sblas

// ---- C ABI ---------------------------------------------------------------------------------------------------------
extern "C" {

size_t sblas_hip_csr_softmax_workspace(int64_t rows, int64_t nnz)
{
    if (rows <= 0 || nnz <= sblas::SM_SUPER) return 0; // no row can be longer than a supercell
    return ((size_t)sblas::softmax_slots(nnz) * 2 * sizeof(double) + 15) / 16 * 16;
}

int sblas_hip_csr_softmax_f64_i32(int dev, void *stream, int64_t rows, int64_t nnz, const int32_t *rowptr, const double *x,
                                  double scale, double *out, void *workspace, size_t workspace_bytes)
{
    bool go;
    if (const int rc = sblas::softmax_args(dev, stream, rows, nnz, rowptr, x, x, out, workspace, workspace_bytes, &go)) return rc;
    if (!go) return SBLAS_OK;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    return sblas::launch_softmax<false>((hipStream_t)stream, (int)rows, (int)nnz, rowptr, x, nullptr, scale, out, workspace) ==
                   hipSuccess
               ? SBLAS_OK
               : SBLAS_E_HIP;
}

int sblas_hip_csr_softmax_backward_f64_i32(int dev, void *stream, int64_t rows, int64_t nnz, const int32_t *rowptr,
                                           const double *p, const double *dp, double scale, double *dx, void *workspace,
                                           size_t workspace_bytes)
{
    bool go;
    if (const int rc = sblas::softmax_args(dev, stream, rows, nnz, rowptr, p, dp, dx, workspace, workspace_bytes, &go)) return rc;
    if (!go) return SBLAS_OK;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    return sblas::launch_softmax<true>((hipStream_t)stream, (int)rows, (int)nnz, rowptr, p, dp, scale, dx, workspace) == hipSuccess
               ? SBLAS_OK
               : SBLAS_E_HIP;
}

} // extern "C"
