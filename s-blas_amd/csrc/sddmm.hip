// sddmm.hip -- SDDMM on a CSR pattern for gfx950 (wave64): out[e] = alpha * <X[row(e), :], Y[col(e), :]> + beta * out[e]
// for every stored entry e, and its C-ABI entry points (include/sblas_hip.h, "SDDMM").  DESIGN.md 3.15.
//
//   sddmm_kernel<G, PASSES, VEC>   a workgroup per run of SDDMM_CHUNK consecutive nonzeros, G lanes per nonzero
//
// Parallel over nonzeros: a workgroup finds the rows of its first and last nonzero by a 256-way search in rowptr, marks
// the row starts that fall inside its run in LDS and turns them into one row index per nonzero with a max-scan (empty
// rows and rows of any length cost the same).  A lane group then walks its share of consecutive nonzeros: the row of X
// stays in registers while the row index does not change, the row of Y of the next nonzero is fetched while the current
// one is multiplied.
//
// Summation order (a function of k alone).  k is cut into slices of SDDMM_SLICE = 128 elements, the last one shorter; a
// slice of kj elements is summed by G = sddmm_group(kj) lanes.  Lane l of a group adds, in this order and with one fma each
// into a sum that starts at +0, the products of the elements 2q and 2q + 1 of its pieces q = l, l + G, l + 2G, ... (a piece
// is two consecutive elements, 16 bytes); elements at or beyond kj are never loaded: their place in the registers holds
// +0 for both factors, and fma(+0, +0, s) returns s (s is never -0: it starts at +0).  The G partial sums are
// then folded in a fixed butterfly, s += s[l ^ 1], s += s[l ^ 2], s += s[l ^ 4], s += s[l ^ 8] (the first log2 G of
// them), after which every lane of the group holds the same bits.  The first slice gives out = alpha * s (beta == 0) or
// fma(beta, out, alpha * s), the epilogue of the SpMM kernels; every later slice, a launch of its own, out = out +
// alpha * s.  Nothing in this depends on the entry's position, its row, the operands' layout or alignment: VEC only widens
// the loads, PASSES only unrolls the piece loop, FULL (k == 2 * G * PASSES: every piece whole) only drops the masks.  (Slices: at k = 256 the rows of Y that the workgroups of one XCD have in
// flight no longer fit its 4 MiB L2 -- the bench matrix's band is 4000 rows of 2 KiB; 128 elements at a time they do.)
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include "../../include/sblas_hip.h"
#include "capi_util.h"
#include "kernels.h"
#include "rowwise.h" // group_sum, load_piece, block_row_of

namespace sblas {

constexpr int SDDMM_THREADS = 256;
constexpr int SDDMM_CHUNK = 1024; // nonzeros per workgroup: four per thread in the row-index scan
// SDDMM_SLICE (elements of k per launch) and sddmm_group (lanes per nonzero for a slice): rowwise.h

// k <= SDDMM_SLICE: one slice.  The piece loop has at most PASSES rounds (k <= 2 * G * PASSES), unrolled.  FULL: k ==
// 2 * G * PASSES, no load is masked (the masks cost a fifth of the time at k = 64).
template <int G, int PASSES, bool VEC, bool FULL>
__global__ __launch_bounds__(SDDMM_THREADS) void sddmm_kernel(int rows, int nnz, int nchunks, const int *__restrict__ rowptr,
                                                               const int *__restrict__ colidx, const double *__restrict__ X,
                                                               int64_t ldx, const double *__restrict__ Y, int64_t ldy, int k,
                                                               double alpha, double beta, double *__restrict__ out)
{
    __shared__ int rowof[SDDMM_CHUNK];
    __shared__ double res[SDDMM_CHUNK];
    __shared__ int wave_max[SDDMM_THREADS / 64];
    const int tid = threadIdx.x;
    const int chunk = xcd_contiguous_panel((int)blockIdx.x, nchunks);
    const int e0 = chunk * SDDMM_CHUNK;
    const int cnt = min(SDDMM_CHUNK, nnz - e0);

    // ---- one row index per nonzero of the run ----
    const int r_lo = block_row_of<SDDMM_THREADS>(rowptr, rows, e0);
    const int r_hi = block_row_of<SDDMM_THREADS>(rowptr, rows, e0 + cnt - 1);
    for (int i = tid; i < SDDMM_CHUNK; i += SDDMM_THREADS) rowof[i] = r_lo;
    __syncthreads();
    for (int64_t r = (int64_t)r_lo + 1 + tid; r <= r_hi; r += SDDMM_THREADS) {
        const int s = rowptr[r] - e0; // in (0, cnt): r_lo is the last row that starts at or before e0
        if (s > 0 && s < cnt) atomicMax(&rowof[s], (int)r); // rows that start together: the last one owns the entry
    }
    __syncthreads();
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
        v.x = max(v.x, before), v.y = max(v.y, before), v.z = max(v.z, before), v.w = max(v.w, before);
        reinterpret_cast<int4 *>(rowof)[tid] = v;
    }
    __syncthreads();

    // ---- the dot products: group g takes the nonzeros [g * EPG, (g + 1) * EPG) of the run ----
    constexpr int NG = SDDMM_THREADS / G, EPG = SDDMM_CHUNK / NG;
    const int l = tid % G, i0 = (tid / G) * EPG;
    const int iend = min(i0 + EPG, cnt);
    // G consecutive column indices per load, one per lane of the group, handed round by lane permutes: a load a nonzero
    // would cost the vector-memory address unit half of what a 64-element row of Y does
    auto cols_at = [&](int i) { return (i + l < iend) ? colidx[e0 + i + l] : 0; };
    auto col_of = [&](int cv, int j) {
        if constexpr (G == 1) return cv;
        else return __shfl(cv, j, G);
    };
    double2 x[PASSES], y[PASSES], yn[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; ++p) x[p] = y[p] = yn[p] = make_double2(0.0, 0.0);
    int rc = -1;
    int cv = cols_at(i0);
    {
        const int c = col_of(cv, 0);
        if (i0 < iend) {
            const double *yrow = Y + (int64_t)c * ldy;
#pragma unroll
            for (int p = 0; p < PASSES; ++p) yn[p] = load_piece<VEC, FULL>(yrow, 2 * (p * G + l), k);
        }
    }
    for (int ib = i0; ib < iend; ib += G) {
        const int cvn = cols_at(ib + G);
        const int jn = min(G, iend - ib);
        for (int j = 0; j < jn; ++j) {
            const int i = ib + j;
#pragma unroll
            for (int p = 0; p < PASSES; ++p) y[p] = yn[p];
            const int cnext = col_of(j + 1 < G ? cv : cvn, (j + 1) & (G - 1));
            if (i + 1 < iend) { // the next nonzero's row of Y, in flight behind this one's arithmetic
                const double *yrow = Y + (int64_t)cnext * ldy;
#pragma unroll
                for (int p = 0; p < PASSES; ++p) yn[p] = load_piece<VEC, FULL>(yrow, 2 * (p * G + l), k);
            }
            const int r = rowof[i];
            if (r != rc) { // the row of X stays in registers while the row index does not change
                const double *xrow = X + (int64_t)r * ldx;
#pragma unroll
                for (int p = 0; p < PASSES; ++p) x[p] = load_piece<VEC, FULL>(xrow, 2 * (p * G + l), k);
                rc = r;
            }
            double s = 0.0;
#pragma unroll
            for (int p = 0; p < PASSES; ++p) {
                s = fma(x[p].x, y[p].x, s); // an element at or beyond k: both factors are the +0 load_piece left
                s = fma(x[p].y, y[p].y, s);
            }
            s = group_sum<G>(s);
            if (l == 0) res[i] = s;
        }
        cv = cvn;
    }
    __syncthreads();
    for (int i = tid; i < cnt; i += SDDMM_THREADS) {
        const double sres = alpha * res[i];
        double *dst = out + e0 + i;
        *dst = (beta == 0.0) ? sres : fma(beta, *dst, sres);
    }
}

template <int G, int PASSES>
static void launch_sddmm_gp(hipStream_t s, bool vec, int nchunks, int rows, int nnz, const int *rowptr, const int *colidx,
                            const double *X, int64_t ldx, const double *Y, int64_t ldy, int k, double alpha, double beta,
                            double *out)
{
    const bool full = k == 2 * G * PASSES; // every piece of every round is whole: no masks
#define SDDMM_K(V, F)                                                                                                          \
    hipLaunchKernelGGL((sddmm_kernel<G, PASSES, V, F>), dim3(nchunks), dim3(SDDMM_THREADS), 0, s, rows, nnz, nchunks, rowptr,   \
                       colidx, X, ldx, Y, ldy, k, alpha, beta, out)
    if (vec && full) SDDMM_K(true, true);
    else if (vec) SDDMM_K(true, false);
    else if (full) SDDMM_K(false, true);
    else SDDMM_K(false, false);
#undef SDDMM_K
}

// X, Y: row-major (rows x k at ldx, cols x k at ldy), read in place, a launch per slice of k (a slice starts 1 KiB into a
// row: the alignment is that of the row).  16-byte loads when both bases and both row strides allow them, 8-byte loads
// otherwise: the same sums either way.
static hipError_t launch_sddmm(hipStream_t s, int rows, int nnz, const int *rowptr, const int *colidx, const double *X,
                               int64_t ldx, const double *Y, int64_t ldy, int k, double alpha, double beta, double *out)
{
    const bool vec = aligned16(X) && aligned16(Y) && ldx % 2 == 0 && ldy % 2 == 0;
    const int nchunks = (nnz + SDDMM_CHUNK - 1) / SDDMM_CHUNK;
#define SDDMM_GO(G, P) launch_sddmm_gp<G, P>(s, vec, nchunks, rows, nnz, rowptr, colidx, X + j0, ldx, Y + j0, ldy, kj, alpha, bj, out)
    for (int j0 = 0; j0 == 0 || j0 < k; j0 += SDDMM_SLICE) { // k == 0: one launch, out = alpha * 0 + beta * out
        const int kj = k - j0 < SDDMM_SLICE ? k - j0 : SDDMM_SLICE;
        const double bj = j0 == 0 ? beta : 1.0;
        const int g = sddmm_group(kj), pz = (kj + 2 * g - 1) / (2 * g); // rounds of pieces: at most 4
        switch (g) {
        case 1: pz <= 1 ? SDDMM_GO(1, 1) : SDDMM_GO(1, 2); break;
        case 2: SDDMM_GO(2, 2); break;
        case 4: pz <= 2 ? SDDMM_GO(4, 2) : SDDMM_GO(4, 4); break;
        case 8: SDDMM_GO(8, 4); break;
        default: SDDMM_GO(16, 4);
        }
    }
#undef SDDMM_GO
    return hipGetLastError();
}

} // namespace sblas

// ---- C ABI ---------------------------------------------------------------------------------------------------------

// leading dimension of the row-major copy of a column-major operand: a width the staging copy has a kernel for
static int64_t sddmm_ldt(int64_t k) { return k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : (k + 7) / 8 * 8; }
// bytes of that copy for an operand of r rows: r + 1 rows (the staging copy writes a zero row behind the last one) and
// its header, a multiple of 256
static size_t sddmm_stage_bytes(int64_t r, int64_t k)
{
    return (((size_t)r + 1) * (size_t)sddmm_ldt(k) * sizeof(double) + sblas::TAIL_HDR * sizeof(int) + 255) / 256 * 256;
}

extern "C" {

size_t sblas_hip_sddmm_csr_workspace(int64_t rows, int64_t cols, int64_t nnz, int64_t k, int order_x, int order_y)
{
    if (rows <= 0 || cols <= 0 || nnz <= 0 || k <= 0) return 0;
    size_t bytes = 0;
    if (order_x == SBLAS_COL_MAJOR) bytes += sddmm_stage_bytes(rows, k);
    if (order_y == SBLAS_COL_MAJOR) bytes += sddmm_stage_bytes(cols, k);
    return bytes;
}

int sblas_hip_sddmm_csr_f64_i32(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr,
                                const int32_t *colidx, const double *X, int64_t ldx, int order_x, const double *Y,
                                int64_t ldy, int order_y, int64_t k, double alpha, double beta, double *out, void *workspace,
                                size_t workspace_bytes)
{
    if (!order_ok(order_x) || !order_ok(order_y)) return SBLAS_E_INVALID;
    if (!csr_args_ok(rows, cols, nnz, rowptr, colidx, out) || k < 0 || k > INT_MAX) return SBLAS_E_INVALID;
    if (!ld_ok(order_x, ldx, rows, k) || !ld_ok(order_y, ldy, cols, k)) return SBLAS_E_INVALID;
    if (nnz == 0) return SBLAS_OK;
    if (rows == 0 || cols == 0) return SBLAS_E_INVALID; // entries without a place
    if (k > 0 && (!X || !Y)) return SBLAS_E_INVALID;
    const bool stage_x = k > 0 && order_x == SBLAS_COL_MAJOR, stage_y = k > 0 && order_y == SBLAS_COL_MAJOR;
    const size_t need = sblas_hip_sddmm_csr_workspace(rows, cols, nnz, k, order_x, order_y);
    if (need > 0 && (!workspace || workspace_bytes < need)) return SBLAS_E_WORKSPACE;
    if (need > 0 && !aligned16(workspace)) return SBLAS_E_INVALID;
    if (sblas::options().validate)
        if (const int vrc = sblas_hip_debug_validate_csr_i32(dev, stream, rows, cols, nnz, rowptr, colidx)) return vrc;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    const hipStream_t s = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    if (stage_x) {
        double *Xt = reinterpret_cast<double *>(ws);
        if (sblas::launch_dense_to_rowmajor(s, rows, k, X, ldx, Xt, sddmm_ldt(k), false) != hipSuccess) return SBLAS_E_HIP;
        X = Xt, ldx = sddmm_ldt(k), ws += sddmm_stage_bytes(rows, k);
    }
    if (stage_y) {
        double *Yt = reinterpret_cast<double *>(ws);
        if (sblas::launch_dense_to_rowmajor(s, cols, k, Y, ldy, Yt, sddmm_ldt(k), false) != hipSuccess) return SBLAS_E_HIP;
        Y = Yt, ldy = sddmm_ldt(k);
    }
    return sblas::launch_sddmm(s, (int)rows, (int)nnz, rowptr, colidx, X, ldx, Y, ldy, (int)k, alpha, beta, out) == hipSuccess
               ? SBLAS_OK
               : SBLAS_E_HIP;
}

} // extern "C"
