// gmres.hip -- right-preconditioned restarted GMRES(m) on a device-resident plan, in the style of
// krylov.hip: start / iterate / status, only status synchronises, no atomics, nothing waits across workgroups, no
// allocation after create, and every bit pinned.  Between two SpMVs (or triangular solves) a step is
//   dots     stage 1 of the dots (v_i, w), i <= j, in ONE pass over memory: a workgroup is a cell, lane t keeps its eight
//            elements of w in registers and walks the columns of V; partial[i * cells + c] has the single dot's bits;
//   fold     stage 2: one workgroup folds the j + 1 dots one after another, and its lane 0 takes what follows from them
//            (h, h + c, or the scalar step of gmres.h: the Givens rotations, |g_{j+1}|, the test, the count, the status);
//   project  w <- w - sum h_i v_i, ascending, which in the second Gram-Schmidt pass is also stage 1 of (w, w);
//   normal   v_{j+1} = w / eta (a rounded division per element) and the vector the next step multiplies: z = v_{j+1},
//            or dinv o v_{j+1} with Jacobi.
// A close forms x from the finished columns (back substitution by one lane, u = sum y_i v_i, z = M^-1 u, x = x + z); a
// restart forms r = b - A x, tests it and begins the next cycle.
//
// The position.  j is NOT a launch argument: every kernel reads the number of finished columns from the scalar block.
// The host only counts steps to know where a close and a restart belong in the chain, so an iterate() captured in a
// graph can be replayed from any position: a step enqueued behind a full cycle does nothing until the chain's next
// close and restart have run.  That is why the next step's operand is a vector of its own (z) and not a pointer into V.
//
// The freeze.  Once the status is not RUNNING every kernel that writes x, V, g, R, c, s, the count or the status returns
// at entry or its lane 0 changes nothing -- except the one close that applies the columns finished so far.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <memory>
#include "../../include/sblas_hip.h"
#include "precond.h"

#pragma clang fp contract(off) // file scope, ahead of gmres.h: a * b + c is two roundings in the scalar step and below

#define GMRES_HD __host__ __device__
#include "gmres.h"
#include "gmres_fold.h" // the fold ops, who acts, the sums, lane 0's part, the close's lane
#include "krylov_fold.h"

using namespace sblas;

namespace {

constexpr int G = GMRES_DOT_GROUP;
constexpr int PL = KRYLOV_PER_LANE;

// how a column kernel learns its column count
enum { MODE_FREE = 0,   // from the launch (the stand-alone entry points, start's (b, b))
       MODE_FIRST = 1,  // a step's first kernels: columns + 1 while RUNNING with the cycle not full, else nothing
       MODE_ACTIVE = 2, // behind a step's first fold: columns + 1 while GS_ACTIVE
       MODE_CLOSE = 3 };// behind a close's first kernel: columns while GS_CLOSE

struct ColArgs {
    int64_t n, cells, ldv;
    int nk, mode;
    const double *V;   // column i at V + i * ldv
    const double *coef; // project: h; combine: y (device)
    double *w;         // dots: read; project: updated; combine: written
    double *part;      // dots: partial[i * cells + c]; project: stage 1 of (w, w), or NULL
    const double *blk;
};

__device__ __forceinline__ int column_count(const double *blk, int mode, int nk)
{
    if (mode == MODE_FREE) return nk;
    const long long *ib = reinterpret_cast<const long long *>(blk); // block-uniform loads, read once
    if (mode == MODE_FIRST) return ib[GS_STATUS] == GMRES_RUNNING && ib[GS_COLS] < ib[GS_M] ? (int)ib[GS_COLS] + 1 : 0;
    if (mode == MODE_ACTIVE) return ib[GS_ACTIVE] ? (int)ib[GS_COLS] + 1 : 0;
    return ib[GS_CLOSE] ? (int)ib[GS_COLS] : 0;
}

// lane t's eight elements of a cell: where they are, which exist (FULL: all), and G columns' worth of them loaded
// together so that their latencies overlap.  A group's surplus columns are clamped to the last one and never used.
template <bool FULL> struct Lane {
    int64_t first;
    bool live[PL];
    __device__ __forceinline__ Lane(int64_t n)
    {
        first = (int64_t)blockIdx.x * KRYLOV_CELL + threadIdx.x;
#pragma unroll
        for (int k = 0; k < PL; ++k) live[k] = FULL || first + k * KRYLOV_LANES < n;
    }
    __device__ __forceinline__ void load(const double *p, double (&v)[PL]) const
    {
#pragma unroll
        for (int k = 0; k < PL; ++k) v[k] = live[k] ? p[first + k * KRYLOV_LANES] : 0.0;
    }
    __device__ __forceinline__ void group(const ColArgs &a, int i0, int nk, double (&v)[G][PL]) const
    {
#pragma unroll
        for (int q = 0; q < G; ++q) {
            const int col = i0 + q < nk ? i0 + q : nk - 1;
            load(a.V + (int64_t)col * a.ldv, v[q]);
        }
    }
    __device__ __forceinline__ void store(double *p, const double (&v)[PL]) const
    {
#pragma unroll
        for (int k = 0; k < PL; ++k)
            if (live[k]) p[first + k * KRYLOV_LANES] = v[k];
    }
};

__device__ __forceinline__ bool full_cell(int64_t n) { return ((int64_t)blockIdx.x + 1) * KRYLOV_CELL <= n; }

// ---- the multi-dot, stage 1 ------------------------------------------------------------------------------------------
// Lane t's sum over its elements in order, the product rounded and then the sum, from +0; the butterfly inside the wave;
// the four waves' sums wait in LDS for the one barrier at the end.  Exactly krylov_dot_kernel's order for every column.
template <bool FULL> __device__ __forceinline__ void dots_cell(const ColArgs &a, int nk, double (*ws)[4])
{
    const Lane<FULL> lane(a.n);
    double wv[PL];
    lane.load(a.w, wv);
    for (int i0 = 0; i0 < nk; i0 += G) {
        double v[G][PL];
        lane.group(a, i0, nk, v);
#pragma unroll
        for (int q = 0; q < G; ++q) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < PL; ++k)
                if (lane.live[k]) acc = acc + v[q][k] * wv[k];
            const double s = wave_fold(acc);
            if ((threadIdx.x & 63) == 0 && i0 + q < nk) ws[i0 + q][threadIdx.x >> 6] = s;
        }
    }
}

__global__ __launch_bounds__(KRYLOV_LANES) void gmres_dots_kernel(const ColArgs a)
{
    __shared__ double ws[GMRES_MAX_DOTS][4];
    const int nk = column_count(a.blk, a.mode, a.nk);
    if (nk <= 0) return;
    if (full_cell(a.n)) dots_cell<true>(a, nk, ws); // only the last cell checks bounds
    else dots_cell<false>(a, nk, ws);
    __syncthreads();
    for (int i = threadIdx.x; i < nk; i += KRYLOV_LANES) a.part[(int64_t)i * a.cells + blockIdx.x] = (ws[i][0] + ws[i][1]) + (ws[i][2] + ws[i][3]);
}

// ---- the projection: w <- w - coef_0 v_0 - coef_1 v_1 - ..., each product rounded and each difference rounded ---------
template <bool FULL> __device__ __forceinline__ void project_cell(const ColArgs &a, int nk)
{
    const Lane<FULL> lane(a.n);
    double t[PL];
    lane.load(a.w, t);
    for (int i0 = 0; i0 < nk; i0 += G) {
        double v[G][PL];
        lane.group(a, i0, nk, v);
#pragma unroll
        for (int q = 0; q < G; ++q) {
            if (i0 + q < nk) { // uniform
                const double hq = a.coef[i0 + q];
#pragma unroll
                for (int k = 0; k < PL; ++k) t[k] = t[k] - hq * v[q][k];
            }
        }
    }
    lane.store(a.w, t);
    if (a.part) { // stage 1 of (w, w) over what was just written
        double acc[1] = {0.0};
#pragma unroll
        for (int k = 0; k < PL; ++k)
            if (lane.live[k]) acc[0] = acc[0] + t[k] * t[k];
        cell_store<1>(acc, a.part, a.cells);
    }
}

__global__ __launch_bounds__(KRYLOV_LANES) void gmres_project_kernel(const ColArgs a)
{
    const int nk = column_count(a.blk, a.mode, a.nk);
    if (nk <= 0) return;
    if (full_cell(a.n)) project_cell<true>(a, nk);
    else project_cell<false>(a, nk);
}

// ---- the combination: u = y_0 v_0, then u = u + y_l v_l ascending, rounded product and rounded sum ----------------------
template <bool FULL> __device__ __forceinline__ void combine_cell(const ColArgs &a, int nk)
{
    const Lane<FULL> lane(a.n);
    double t[PL];
    for (int i0 = 0; i0 < nk; i0 += G) {
        double v[G][PL];
        lane.group(a, i0, nk, v);
#pragma unroll
        for (int q = 0; q < G; ++q) {
            if (i0 + q < nk) {
                const double yq = a.coef[i0 + q];
                if (i0 + q == 0) {
#pragma unroll
                    for (int k = 0; k < PL; ++k) t[k] = yq * v[q][k];
                } else {
#pragma unroll
                    for (int k = 0; k < PL; ++k) t[k] = t[k] + yq * v[q][k];
                }
            }
        }
    }
    lane.store(a.w, t);
}

__global__ __launch_bounds__(KRYLOV_LANES) void gmres_combine_kernel(const ColArgs a)
{
    const int nk = column_count(a.blk, a.mode, a.nk);
    if (nk <= 0) return;
    if (full_cell(a.n)) combine_cell<true>(a, nk);
    else combine_cell<false>(a, nk);
}

// ---- the plan's elementwise passes -------------------------------------------------------------------------------------
struct VecArgs {
    int64_t n, cells, ldv;
    double *blk, *part;
    double *V, *w, *z, *x;
    const double *b, *dinv, *u;
};

// r = b - w (w = A x on entry), one rounded difference, left in w; stage 1 of (r, r).  START: b == 0 writes x = 0 and
// r = 0 instead, and the status is not asked.  Otherwise: only as a restart is due.
template <bool START> __global__ __launch_bounds__(KRYLOV_LANES) void gmres_residual_kernel(const VecArgs a)
{
    const long long *ib = reinterpret_cast<const long long *>(a.blk);
    if (!START && (ib[GS_STATUS] != GMRES_RUNNING || ib[GS_COLS] != ib[GS_M] || ib[GS_PENDING] != 0)) return;
    const bool zero_x = START && ib[GS_ZERO_X] != 0;
    double acc[1] = {0.0};
    cell_walk(a.n, [&](int64_t i) {
        if (zero_x) a.x[i] = 0.0;
        const double ri = zero_x ? 0.0 : a.b[i] - a.w[i];
        a.w[i] = ri;
        acc[0] = acc[0] + ri * ri;
    });
    cell_store<1>(acc, a.part, a.cells);
}

// v_k = w / eta with k and eta from the block, and the next step's operand z = v_k (JAC: dinv o v_k)
template <bool JAC> __global__ __launch_bounds__(KRYLOV_LANES) void gmres_normal_kernel(const VecArgs a)
{
    const long long *ib = reinterpret_cast<const long long *>(a.blk);
    if (!ib[GS_ACTIVE]) return;
    const double eta = a.blk[GS_ETA];
    double *v = a.V + ib[GS_COLS] * a.ldv;
    cell_walk(a.n, [&](int64_t i) {
        const double vi = a.w[i] / eta;
        v[i] = vi;
        a.z[i] = JAC ? a.dinv[i] * vi : vi;
    });
}

// x = x + z with z = u (JAC: the rounded dinv o u), when this close acts
template <bool JAC> __global__ __launch_bounds__(KRYLOV_LANES) void gmres_x_kernel(const VecArgs a)
{
    const long long *ib = reinterpret_cast<const long long *>(a.blk);
    if (!ib[GS_CLOSE]) return;
    cell_walk(a.n, [&](int64_t i) {
        const double zi = JAC ? a.dinv[i] * a.u[i] : a.u[i];
        a.x[i] = a.x[i] + zi;
    });
}

// the first kernel of a close: does it act, and if so y from R y = g over the finished columns
__global__ void gmres_close_kernel(double *blk, double *mat)
{
    if (threadIdx.x != 0) return;
    gmres_close_lane(blk, mat);
}

// ---- stage 2, which is also the scalar step (gmres_fold.h) -------------------------------------------------------------
__global__ __launch_bounds__(KRYLOV_LANES) void gmres_fold_kernel(int op, int nd, int64_t cells, const double *part, double *blk, double *mat,
                                                                 double *out, double rtol, double atol, long long max_iter, int m)
{
    __shared__ double ws[GMRES_MAX_DOTS][4];
    long long *ib = reinterpret_cast<long long *>(blk);
    if (!gmres_fold_acts(op, ib)) return;
    if (op == GF_H1 || op == GF_H2) nd = (int)ib[GS_COLS] + 1;
    gmres_fold_sums(nd, cells, part, cells, ws);
    __syncthreads();
    if (threadIdx.x != 0) return;
    gmres_fold_lane0(op, nd, ws, blk, mat, out, 1, rtol, atol, max_iter, m);
}

// ---- launches ----------------------------------------------------------------------------------------------------------
struct GmresPlan {
    int dev = -1, m = 0;
    int64_t n = 0, nnz = 0, cells = 0, ldv = 0;
    const int32_t *rowptr = nullptr, *colidx = nullptr; // the caller's
    const void *spmv = nullptr;
    PrecondSeat pre; // start() gives it the caller's values
    int n_vectors = 0;
    size_t vector_bytes = 0, partial_bytes = 0, bytes = 0;
    DeviceBuffer buf; // block | small matrices | partials | V, w, u, z [, the solves' temporary]
    double *blk = nullptr, *mat = nullptr, *part = nullptr, *vec = nullptr;
    // one solve: start() keeps what iterate() needs
    bool started = false;
    int pos = 0; // steps enqueued since the chain's last restart (or start): where the next close and restart belong
    const double *val = nullptr, *b = nullptr;
    double *x = nullptr;
    double *col(int k) const { return vec + (size_t)k * (size_t)ldv; }
    double *w() const { return col(m + 1); }
    double *u() const { return col(m + 2); }
    double *z() const { return col(m + 3); }
    double *tmp() const { return col(m + 4); }
};

void fold(const GmresPlan *p, hipStream_t s, int op, double rtol = 0.0, double atol = 0.0, int64_t max_iter = 0)
{
    gmres_fold_kernel<<<1, KRYLOV_LANES, 0, s>>>(op, 1, p->cells, p->part, p->blk, p->mat, nullptr, rtol, atol, (long long)max_iter, p->m);
}

ColArgs col_args(const GmresPlan *p, int mode, const double *coef, double *w, double *part)
{
    return ColArgs{p->n, p->cells, p->ldv, 0, mode, p->vec, coef, w, part, p->blk};
}

VecArgs vec_args(const GmresPlan *p)
{
    return VecArgs{p->n, p->cells, p->ldv, p->blk, p->part, p->vec, p->w(), p->z(), p->x, p->b, p->pre.values, p->u()};
}

void normalise(const GmresPlan *p, hipStream_t s)
{
    const unsigned grid = (unsigned)p->cells;
    if (p->pre.jacobi()) gmres_normal_kernel<true><<<grid, KRYLOV_LANES, 0, s>>>(vec_args(p));
    else gmres_normal_kernel<false><<<grid, KRYLOV_LANES, 0, s>>>(vec_args(p));
}

int gmres_step_launches(const GmresPlan *p, hipStream_t s)
{
    const unsigned grid = (unsigned)p->cells;
    const bool ilu = p->pre.applied();
    int rc;
    if (ilu && (rc = p->pre.apply(s, p->z(), p->tmp(), p->u())) != SBLAS_OK) return rc; // u is free between two closes
    if ((rc = plan_spmv(p, s, ilu ? p->u() : p->z(), p->w())) != SBLAS_OK) return rc;
    gmres_dots_kernel<<<grid, KRYLOV_LANES, 0, s>>>(col_args(p, MODE_FIRST, nullptr, p->w(), p->part));
    fold(p, s, GF_H1);
    gmres_project_kernel<<<grid, KRYLOV_LANES, 0, s>>>(col_args(p, MODE_ACTIVE, p->mat + GM_H, p->w(), nullptr));
    gmres_dots_kernel<<<grid, KRYLOV_LANES, 0, s>>>(col_args(p, MODE_ACTIVE, nullptr, p->w(), p->part));
    fold(p, s, GF_H2);
    gmres_project_kernel<<<grid, KRYLOV_LANES, 0, s>>>(col_args(p, MODE_ACTIVE, p->mat + GM_H2, p->w(), p->part));
    fold(p, s, GF_STEP);
    normalise(p, s);
    return SBLAS_OK;
}

int gmres_close_launches(const GmresPlan *p, hipStream_t s)
{
    const unsigned grid = (unsigned)p->cells;
    gmres_close_kernel<<<1, 64, 0, s>>>(p->blk, p->mat);
    gmres_combine_kernel<<<grid, KRYLOV_LANES, 0, s>>>(col_args(p, MODE_CLOSE, p->mat + GM_Y, p->u(), nullptr));
    VecArgs a = vec_args(p);
    if (p->pre.applied()) { // in place where M^-1 may run so; else the correction is read from the temporary
        double *out = p->pre.in_place() ? p->u() : p->tmp();
        const int rc = p->pre.apply(s, p->u(), p->tmp(), out);
        if (rc != SBLAS_OK) return rc;
        a.u = out;
    }
    if (p->pre.jacobi()) gmres_x_kernel<true><<<grid, KRYLOV_LANES, 0, s>>>(a);
    else gmres_x_kernel<false><<<grid, KRYLOV_LANES, 0, s>>>(a);
    return SBLAS_OK;
}

int gmres_restart_launches(const GmresPlan *p, hipStream_t s)
{
    const int rc = plan_spmv(p, s, p->x, p->w());
    if (rc != SBLAS_OK) return rc;
    gmres_residual_kernel<false><<<(unsigned)p->cells, KRYLOV_LANES, 0, s>>>(vec_args(p));
    fold(p, s, GF_BEGIN_RESTART);
    normalise(p, s);
    return SBLAS_OK;
}

bool columns_ok(int64_t n, int k, const double *V, int64_t ldv, const void *a, const void *b)
{
    if (n < 0 || n > INT_MAX || k < 1 || k > GMRES_MAX_DOTS || !a) return false;
    if (k > 1 && ldv < n) return false;
    return n == 0 || (V && b);
}

} // namespace

extern "C" {

size_t sblas_hip_gmres_dots_workspace(int64_t n, int k)
{
    if (n < 0 || k < 1 || k > GMRES_MAX_DOTS) return 0;
    const size_t sums = (size_t)k * (size_t)krylov_cells(n);
    return (sums ? sums : 1) * sizeof(double); // never 0: a workspace is always asked for
}

int sblas_hip_gmres_dots_f64(int dev, void *stream, int64_t n, int k, const double *V, int64_t ldv, const double *w, double *out,
                             void *workspace, size_t workspace_bytes)
{
    if (!columns_ok(n, k, V, ldv, out, w)) return SBLAS_E_INVALID;
    if (!workspace || workspace_bytes < sblas_hip_gmres_dots_workspace(n, k)) return SBLAS_E_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 7u) return SBLAS_E_INVALID;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    hipStream_t s = (hipStream_t)stream;
    const int64_t cells = krylov_cells(n);
    double *part = static_cast<double *>(workspace);
    if (cells > 0)
        gmres_dots_kernel<<<(unsigned)cells, KRYLOV_LANES, 0, s>>>(ColArgs{n, cells, ldv, k, MODE_FREE, V, nullptr, const_cast<double *>(w), part, nullptr});
    gmres_fold_kernel<<<1, KRYLOV_LANES, 0, s>>>(GF_OUT, k, cells, part, nullptr, nullptr, out, 0.0, 0.0, 0, 0);
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_gmres_project_f64(int dev, void *stream, int64_t n, int k, const double *V, int64_t ldv, const double *h, double *w,
                                double *partial)
{
    if (!columns_ok(n, k, V, ldv, h, w)) return SBLAS_E_INVALID;
    if (n == 0) return SBLAS_OK;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    const int64_t cells = krylov_cells(n);
    gmres_project_kernel<<<(unsigned)cells, KRYLOV_LANES, 0, (hipStream_t)stream>>>(ColArgs{n, cells, ldv, k, MODE_FREE, V, h, w, partial, nullptr});
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_gmres_combine_f64(int dev, void *stream, int64_t n, int k, const double *V, int64_t ldv, const double *y, double *u)
{
    if (!columns_ok(n, k, V, ldv, y, u)) return SBLAS_E_INVALID;
    if (n == 0) return SBLAS_OK;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    const int64_t cells = krylov_cells(n);
    gmres_combine_kernel<<<(unsigned)cells, KRYLOV_LANES, 0, (hipStream_t)stream>>>(ColArgs{n, cells, ldv, k, MODE_FREE, V, y, u, nullptr, nullptr});
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_gmres_plan_create(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx, int restart,
                                const void *spmv_plan, int precond, const void *lower_plan, const void *upper_plan, void **plan_out)
{
    if (!plan_out) return SBLAS_E_INVALID;
    *plan_out = nullptr;
    if (restart < 1 || restart > GMRES_MAX_RESTART) return SBLAS_E_INVALID;
    if (!precond_known(precond)) return SBLAS_E_INVALID;
    if (n < 0 || nnz < 0 || n > INT_MAX - 64 || nnz > INT_MAX) return SBLAS_E_INVALID;
    if (!rowptr || (nnz > 0 && !colidx) || (n == 0 && nnz != 0)) return SBLAS_E_INVALID;
    const int device = resolve_device(dev);
    if (spmv_plan && sblas_hip_spmv_plan_speaks_for(spmv_plan, device, n, n, nnz, rowptr, colidx) != SBLAS_OK) return SBLAS_E_INVALID;
    std::unique_ptr<GmresPlan> p(new GmresPlan);
    if (p->pre.bind(precond, lower_plan, upper_plan, device, n, nnz, rowptr, colidx) != SBLAS_OK) return SBLAS_E_INVALID;
    p->dev = device, p->m = restart, p->n = n, p->nnz = nnz, p->cells = krylov_cells(n);
    p->rowptr = rowptr, p->colidx = colidx, p->spmv = spmv_plan;
    p->n_vectors = restart + 1 + GMRES_EXTRA_VECTORS + p->pre.applied();
    if (n == 0) {
        *plan_out = p.release();
        return SBLAS_OK;
    }
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    const size_t block_bytes = pad256(GMRES_BLOCK_SLOTS * 8), matrix_bytes = pad256((size_t)GMRES_MATRIX_DOUBLES * 8);
    p->vector_bytes = pad256((size_t)n * 8), p->ldv = (int64_t)(p->vector_bytes / 8);
    p->partial_bytes = pad256((size_t)(restart + 1) * (size_t)p->cells * 8);
    p->bytes = block_bytes + matrix_bytes + p->partial_bytes + (size_t)p->n_vectors * p->vector_bytes;
    if (p->buf.alloc(p->dev, p->bytes) != hipSuccess) return SBLAS_E_HIP;
    // the one moment the buffer is written outside a solve: a close that does not act still runs its M^-1 over u
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(p->buf.at<char>(), 0, p->bytes, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return SBLAS_E_HIP;
    p->blk = p->buf.at<double>(), p->mat = p->buf.at<double>(block_bytes), p->part = p->buf.at<double>(block_bytes + matrix_bytes);
    p->vec = p->buf.at<double>(block_bytes + matrix_bytes + p->partial_bytes);
    *plan_out = p.release();
    return SBLAS_OK;
}

int sblas_hip_gmres_plan_info(const void *plan, int64_t out[14])
{
    if (!plan || !out) return SBLAS_E_INVALID;
    const GmresPlan *p = static_cast<const GmresPlan *>(plan);
    int64_t lower[12], upper[12], launches[4] = {0};
    p->pre.info(lower, upper);
    out[0] = p->n, out[1] = p->nnz, out[2] = p->m, out[3] = p->pre.kind, out[4] = p->n_vectors, out[5] = (int64_t)p->vector_bytes;
    out[6] = (int64_t)p->partial_bytes, out[7] = GMRES_BLOCK_SLOTS * 8, out[8] = (int64_t)GMRES_MATRIX_DOUBLES * 8, out[9] = (int64_t)p->bytes;
    out[13] = sblas_gmres_launches(p->m, p->pre.kind, lower, upper, launches);
    out[10] = launches[0], out[11] = launches[1], out[12] = launches[2];
    return SBLAS_OK;
}

int sblas_hip_gmres_plan_destroy(void *plan)
{
    delete static_cast<GmresPlan *>(plan);
    return SBLAS_OK;
}

int sblas_hip_gmres_start(void *plan, void *stream, const double *val, const double *lu_or_dinv, const double *b, double *x, double rtol,
                          double atol, int64_t max_iter)
{
    GmresPlan *p = static_cast<GmresPlan *>(plan);
    if (!p) return SBLAS_E_INVALID;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    if (!(rtol >= 0.0) || !(atol >= 0.0) || max_iter < 0) return SBLAS_E_INVALID; // a NaN tolerance is refused too
    p->started = false;
    if (p->n == 0) {
        p->started = true;
        return SBLAS_OK;
    }
    if (!b || !x || (p->nnz > 0 && !val) || !p->pre.take(lu_or_dinv)) return SBLAS_E_INVALID;
    p->val = val, p->b = b, p->x = x, p->pos = 0;
    hipStream_t s = (hipStream_t)stream;
    const unsigned grid = (unsigned)p->cells;
    // (b, b) by the multi-dot of one column: the single dot's bits
    gmres_dots_kernel<<<grid, KRYLOV_LANES, 0, s>>>(ColArgs{p->n, p->cells, p->ldv, 1, MODE_FREE, b, nullptr, const_cast<double *>(b), p->part, nullptr});
    fold(p, s, GF_START_B, rtol, atol, max_iter);
    const int rc = plan_spmv(p, s, x, p->w());
    if (rc != SBLAS_OK) return rc;
    gmres_residual_kernel<true><<<grid, KRYLOV_LANES, 0, s>>>(vec_args(p));
    fold(p, s, GF_BEGIN_START);
    normalise(p, s);
    if (hipGetLastError() != hipSuccess) return SBLAS_E_HIP;
    p->started = true;
    return SBLAS_OK;
}

int sblas_hip_gmres_iterate(void *plan, void *stream, int64_t k)
{
    GmresPlan *p = static_cast<GmresPlan *>(plan);
    if (!p || k < 0 || !p->started) return SBLAS_E_INVALID;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    if (p->n == 0) return SBLAS_OK;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    for (int64_t it = 0; it < k; ++it) {
        if ((rc = gmres_step_launches(p, s)) != SBLAS_OK) return rc;
        if (++p->pos == p->m) { // the cycle is full (or the device is frozen and ignores all this)
            p->pos = 0;
            if ((rc = gmres_close_launches(p, s)) != SBLAS_OK || (rc = gmres_restart_launches(p, s)) != SBLAS_OK) return rc;
        }
    }
    if ((rc = gmres_close_launches(p, s)) != SBLAS_OK) return rc; // acts only if the solve ended inside this batch
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_gmres_status(const void *plan, void *stream, double out[8])
{
    const GmresPlan *p = static_cast<const GmresPlan *>(plan);
    if (!p || !out || !p->started) return SBLAS_E_INVALID;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    for (int q = 0; q < 8; ++q) out[q] = 0.0;
    if (p->n == 0) {
        out[0] = SBLAS_KRYLOV_CONVERGED;
        return SBLAS_OK;
    }
    double h[GMRES_BLOCK_SLOTS];
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(h, p->blk, sizeof h, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return SBLAS_E_HIP;
    long long ih[GMRES_BLOCK_SLOTS];
    memcpy(ih, h, sizeof ih);
    out[0] = (double)ih[GS_STATUS], out[1] = (double)ih[GS_ITER], out[2] = h[GS_RNORM], out[3] = h[GS_BNORM];
    out[4] = (double)ih[GS_RESTARTS], out[5] = (double)ih[GS_COLS], out[6] = h[GS_ETA], out[7] = (double)ih[GS_WHICH];
    return SBLAS_OK;
}

} // extern "C"
