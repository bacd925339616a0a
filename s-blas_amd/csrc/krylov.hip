// krylov.hip -- device-resident Krylov solvers on a plan: PCG and BiCGStab.  Everything a solver does
// between two SpMVs (or triangular solves) is one of three kernels:
//   dot     stage 1 of up to KRYLOV_MAX_DOTS dot products in one pass over memory: one workgroup a cell of KRYLOV_CELL
//           elements, the cell's sum to partial[c];
//   update  a fused elementwise update of the recurrence's vectors, which is also stage 1 of the dots of what it wrote;
//   fold    stage 2: ONE workgroup folds the cells' sums and its lane 0 takes the scalar step that follows from them
//           (alpha, beta, omega, |r|, the stopping test, the iteration count, the status word), in the device scalar block.
// Nothing waits across workgroups: no flag polling, no cooperative launch, no atomics.  The only synchronisation is the
// kernel boundary and __syncthreads().  The host passes no scalar of the recurrence and reads none back before status().
//
// The freeze.  Once the status word is not RUNNING, every update kernel returns at entry (the flag is one uniform load,
// read once) and lane 0 of every fold changes nothing.  So x, r, the iteration count and |r| stay exactly what they were
// when the test was met, however many further iterations were already enqueued; the SpMVs, solves and dot stages of those
// iterations still run, into work vectors and partials only.
//
// Arithmetic.  Every product and every sum is rounded on its own: this file is compiled with contraction off, so no
// multiply-add is fused, in the dots or in the updates, and a numpy expression of the same shape reproduces the bits.
// The order of a dot's additions is a function of n alone (include/sblas_hip.h; sblas_krylov_dot_ref restates it): a
// cell is a workgroup whatever the device, so neither the grid nor the CU count can reach it.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <initializer_list>
#include <memory>
#include "../../include/sblas_hip.h"
#include "krylov.h"
#include "precond.h"

#pragma clang fp contract(off) // file scope: a * b + c below is two roundings on every path

#include "krylov_fold.h"   // wave_fold, group_fold, cell_walk, cell_store: shared with gmres.hip and krylov_multi.hip
#include "krylov_scalar.h" // the fold ops and lane 0's scalar step: shared with krylov_multi.hip

using namespace sblas;

namespace {

// internal update ops, after the public SBLAS_KRYLOV_UP_* ones
enum { UP_COPY = 5, UP_START_PCG = 6, UP_START_BICG = 7 };
struct UpArgs {
    int64_t n, cells;
    double *blk;  // the scalar block
    double *part; // cells' sums: dot k of the pass at part[k * cells + c]
    double *v[8];
};

struct DotArgs {
    int64_t n, cells;
    const double *x[KRYLOV_MAX_DOTS], *y[KRYLOV_MAX_DOTS];
    double *part;
};

// ---- dot, stage 1 ----------------------------------------------------------------------------------------------------
template <int ND> __global__ __launch_bounds__(KRYLOV_LANES) void krylov_dot_kernel(const DotArgs a)
{
    double acc[ND];
#pragma unroll
    for (int q = 0; q < ND; ++q) acc[q] = 0.0;
    cell_walk(a.n, [&](int64_t i) {
#pragma unroll
        for (int q = 0; q < ND; ++q) acc[q] = acc[q] + a.x[q][i] * a.y[q][i];
    });
    cell_store<ND>(acc, a.part, a.cells);
}

// ---- the fused updates -----------------------------------------------------------------------------------------------
// JAC: the Jacobi preconditioner rides in the same pass (z = dinv o r, and its partials).  Vectors are not __restrict__:
// without a preconditioner z is r, and p^, s^ are p, s.
template <int OP, bool JAC> __global__ __launch_bounds__(KRYLOV_LANES) void krylov_update_kernel(const UpArgs a)
{
    const long long *ib = reinterpret_cast<const long long *>(a.blk);
    constexpr bool START = OP == UP_START_PCG || OP == UP_START_BICG;
    if (!START && ib[KS_STATUS] != SBLAS_KRYLOV_RUNNING) return; // block-uniform, read once: the freeze
    const double al = a.blk[KS_ALPHA], be = a.blk[KS_BETA], om = a.blk[KS_OMEGA];
    const bool zero_x = START && ib[KS_ZERO_X] != 0;
    double *const *v = a.v;
    if constexpr (OP == SBLAS_KRYLOV_UP_PCG_XR) { // x, r, p, q, dinv, z
        double acc[JAC ? 2 : 1] = {};
        cell_walk(a.n, [&](int64_t i) {
            v[0][i] = v[0][i] + al * v[2][i];
            const double ri = v[1][i] - al * v[3][i];
            v[1][i] = ri;
            acc[0] = acc[0] + ri * ri;
            if constexpr (JAC) {
                const double zi = v[4][i] * ri;
                v[5][i] = zi;
                acc[1] = acc[1] + ri * zi;
            }
        });
        cell_store<JAC ? 2 : 1>(acc, a.part, a.cells);
    } else if constexpr (OP == SBLAS_KRYLOV_UP_PCG_P) { // p, z
        cell_walk(a.n, [&](int64_t i) { v[0][i] = v[1][i] + be * v[0][i]; });
    } else if constexpr (OP == UP_COPY) { // dst, src
        cell_walk(a.n, [&](int64_t i) { v[0][i] = v[1][i]; });
    } else if constexpr (OP == SBLAS_KRYLOV_UP_BICG_P) { // p, r, v, dinv, p^
        cell_walk(a.n, [&](int64_t i) {
            const double pi = v[1][i] + be * (v[0][i] - om * v[2][i]);
            v[0][i] = pi;
            if constexpr (JAC) v[4][i] = v[3][i] * pi;
        });
    } else if constexpr (OP == SBLAS_KRYLOV_UP_BICG_S) { // s, r, v, dinv, s^
        cell_walk(a.n, [&](int64_t i) {
            const double si = v[1][i] - al * v[2][i];
            v[0][i] = si;
            if constexpr (JAC) v[4][i] = v[3][i] * si;
        });
    } else if constexpr (OP == SBLAS_KRYLOV_UP_BICG_XR) { // x, r, p^, s^, s, t, r^
        double acc[2] = {};
        cell_walk(a.n, [&](int64_t i) {
            v[0][i] = (v[0][i] + al * v[2][i]) + om * v[3][i];
            const double ri = v[4][i] - om * v[5][i];
            v[1][i] = ri;
            acc[0] = acc[0] + ri * ri;
            acc[1] = acc[1] + v[6][i] * ri;
        });
        cell_store<2>(acc, a.part, a.cells);
    } else if constexpr (OP == UP_START_PCG) { // r, b, q (= A x0), dinv, z, x
        double acc[JAC ? 2 : 1] = {};
        cell_walk(a.n, [&](int64_t i) {
            if (zero_x) v[5][i] = 0.0; // b == 0: x = 0, and b - A x0 is not formed
            const double ri = zero_x ? 0.0 : v[1][i] - v[2][i];
            v[0][i] = ri;
            acc[0] = acc[0] + ri * ri;
            if constexpr (JAC) {
                const double zi = zero_x ? 0.0 : v[3][i] * ri;
                v[4][i] = zi;
                acc[1] = acc[1] + ri * zi;
            }
        });
        cell_store<JAC ? 2 : 1>(acc, a.part, a.cells);
    } else { // UP_START_BICG: r, b, v (= A x0 on entry, 0 on exit), r^, p, x
        double acc[1] = {};
        cell_walk(a.n, [&](int64_t i) {
            if (zero_x) v[5][i] = 0.0;
            const double ri = zero_x ? 0.0 : v[1][i] - v[2][i];
            v[0][i] = ri, v[3][i] = ri, v[4][i] = 0.0, v[2][i] = 0.0;
            acc[0] = acc[0] + ri * ri;
        });
        cell_store<1>(acc, a.part, a.cells);
    }
}

// ---- stage 2, which is also the scalar step ----------------------------------------------------------------------------
__global__ __launch_bounds__(KRYLOV_LANES) void krylov_fold_kernel(int op, int nd, int flag, int64_t cells, const double *part, double *blk,
                                                                  double rtol, double atol, long long max_iter)
{
    double d[KRYLOV_MAX_DOTS];
    cells_fold(nd, cells, part, cells, d);
    if (threadIdx.x != 0) return;
    if (op == FOLD_OUT) {
        for (int q = 0; q < nd; ++q) blk[q] = d[q];
        return;
    }
    krylov_scalar_step(op, nd, flag, d, blk, rtol, atol, max_iter); // krylov_scalar.h: the one text of the step
}

// ---- launches ----------------------------------------------------------------------------------------------------------
inline void launch_dot(hipStream_t s, int nd, const DotArgs &a)
{
    const unsigned grid = (unsigned)a.cells;
    if (nd == 1) krylov_dot_kernel<1><<<grid, KRYLOV_LANES, 0, s>>>(a);
    else if (nd == 2) krylov_dot_kernel<2><<<grid, KRYLOV_LANES, 0, s>>>(a);
    else krylov_dot_kernel<3><<<grid, KRYLOV_LANES, 0, s>>>(a);
}

inline void launch_fold(hipStream_t s, int op, int nd, int flag, int64_t cells, const double *part, double *blk, double rtol = 0.0,
                        double atol = 0.0, int64_t max_iter = 0)
{
    krylov_fold_kernel<<<1, KRYLOV_LANES, 0, s>>>(op, nd, flag, cells, part, blk, rtol, atol, (long long)max_iter);
}

template <int OP> inline void launch_update_op(hipStream_t s, bool jac, const UpArgs &a)
{
    const unsigned grid = (unsigned)a.cells;
    if (jac) krylov_update_kernel<OP, true><<<grid, KRYLOV_LANES, 0, s>>>(a);
    else krylov_update_kernel<OP, false><<<grid, KRYLOV_LANES, 0, s>>>(a);
}

inline void launch_update(hipStream_t s, int op, bool jac, const UpArgs &a)
{
    switch (op) {
    case SBLAS_KRYLOV_UP_PCG_XR: return launch_update_op<SBLAS_KRYLOV_UP_PCG_XR>(s, jac, a);
    case SBLAS_KRYLOV_UP_PCG_P: return launch_update_op<SBLAS_KRYLOV_UP_PCG_P>(s, false, a);
    case SBLAS_KRYLOV_UP_BICG_P: return launch_update_op<SBLAS_KRYLOV_UP_BICG_P>(s, jac, a);
    case SBLAS_KRYLOV_UP_BICG_S: return launch_update_op<SBLAS_KRYLOV_UP_BICG_S>(s, jac, a);
    case SBLAS_KRYLOV_UP_BICG_XR: return launch_update_op<SBLAS_KRYLOV_UP_BICG_XR>(s, false, a);
    case UP_COPY: return launch_update_op<UP_COPY>(s, false, a);
    case UP_START_PCG: return launch_update_op<UP_START_PCG>(s, jac, a);
    default: return launch_update_op<UP_START_BICG>(s, false, a);
    }
}

struct KrylovPlan {
    int dev = -1, method = 0;
    int64_t n = 0, nnz = 0, cells = 0;
    const int32_t *rowptr = nullptr, *colidx = nullptr; // the caller's
    const void *spmv = nullptr;
    PrecondSeat pre; // start() gives it the caller's values
    int n_vectors = 0;
    size_t vector_bytes = 0, partial_bytes = 0, bytes = 0;
    DeviceBuffer buf; // block | partials | vectors
    double *blk = nullptr, *part = nullptr, *vec = nullptr;
    // one solve: start() keeps what iterate() needs
    bool started = false;
    const double *val = nullptr;
    double *x = nullptr;
    double *w(int k) const { return vec + (size_t)k * (vector_bytes / 8); }
};

// vectors of the plan, by slot
enum { V_R = 0, V_P = 1, V_Q = 2, V_Z = 3, V_TMP_PCG = 4 };
enum { B_R = 0, B_RHAT = 1, B_P = 2, B_V = 3, B_S = 4, B_T = 5, B_PH = 6, B_SH = 7, B_TMP = 8 };

UpArgs up_args(const KrylovPlan *p, std::initializer_list<double *> v)
{
    UpArgs a{p->n, p->cells, p->blk, p->part, {}};
    int k = 0;
    for (double *q : v) a.v[k++] = q;
    return a;
}

void dot(const KrylovPlan *p, hipStream_t s, const double *x0, const double *y0, const double *x1 = nullptr, const double *y1 = nullptr,
         const double *x2 = nullptr, const double *y2 = nullptr)
{
    DotArgs a{p->n, p->cells, {x0, x1, x2}, {y0, y1, y2}, p->part};
    launch_dot(s, x2 ? 3 : x1 ? 2 : 1, a);
}

int pcg_iteration(const KrylovPlan *p, hipStream_t s)
{
    const bool jac = p->pre.jacobi(), ilu = p->pre.applied();
    double *r = p->w(V_R), *pp = p->w(V_P), *q = p->w(V_Q), *z = p->pre.none() ? r : p->w(V_Z);
    int rc = plan_spmv(p, s, pp, q);
    if (rc != SBLAS_OK) return rc;
    dot(p, s, pp, q);
    launch_fold(s, FOLD_PCG_ALPHA, 1, 0, p->cells, p->part, p->blk);
    launch_update(s, SBLAS_KRYLOV_UP_PCG_XR, jac, up_args(p, {p->x, r, pp, q, const_cast<double *>(p->pre.values), z}));
    launch_fold(s, FOLD_PCG_RES, jac ? 2 : 1, !ilu, p->cells, p->part, p->blk);
    if (ilu) {
        if ((rc = p->pre.apply(s, r, p->w(V_TMP_PCG), z)) != SBLAS_OK) return rc;
        dot(p, s, r, z);
        launch_fold(s, FOLD_PCG_BETA, 1, 0, p->cells, p->part, p->blk);
    }
    launch_update(s, SBLAS_KRYLOV_UP_PCG_P, false, up_args(p, {pp, z}));
    return SBLAS_OK;
}

int bicgstab_iteration(const KrylovPlan *p, hipStream_t s)
{
    const bool jac = p->pre.jacobi(), none = p->pre.none(), ilu = p->pre.applied();
    double *r = p->w(B_R), *rh = p->w(B_RHAT), *pp = p->w(B_P), *v = p->w(B_V), *sv = p->w(B_S), *t = p->w(B_T);
    double *ph = none ? pp : p->w(B_PH), *sh = none ? sv : p->w(B_SH), *dinv = const_cast<double *>(p->pre.values);
    int rc;
    launch_update(s, SBLAS_KRYLOV_UP_BICG_P, jac, up_args(p, {pp, r, v, dinv, ph}));
    if (ilu && (rc = p->pre.apply(s, pp, p->w(B_TMP), ph)) != SBLAS_OK) return rc;
    if ((rc = plan_spmv(p, s, ph, v)) != SBLAS_OK) return rc;
    dot(p, s, rh, v);
    launch_fold(s, FOLD_BICG_ALPHA, 1, 0, p->cells, p->part, p->blk);
    launch_update(s, SBLAS_KRYLOV_UP_BICG_S, jac, up_args(p, {sv, r, v, dinv, sh}));
    if (ilu && (rc = p->pre.apply(s, sv, p->w(B_TMP), sh)) != SBLAS_OK) return rc;
    if ((rc = plan_spmv(p, s, sh, t)) != SBLAS_OK) return rc;
    dot(p, s, t, sv, t, t, sv, sv);
    launch_fold(s, FOLD_BICG_OMEGA, 3, 0, p->cells, p->part, p->blk);
    launch_update(s, SBLAS_KRYLOV_UP_BICG_XR, false, up_args(p, {p->x, r, ph, sh, sv, t, rh}));
    launch_fold(s, FOLD_BICG_RES, 2, 0, p->cells, p->part, p->blk);
    return SBLAS_OK;
}

} // namespace

extern "C" {

size_t sblas_hip_krylov_dot_workspace(int64_t n, int ndots)
{
    if (n < 0 || ndots < 1 || ndots > KRYLOV_MAX_DOTS) return 0;
    const size_t sums = (size_t)ndots * (size_t)krylov_cells(n);
    return (sums ? sums : 1) * sizeof(double); // never 0: a workspace is always asked for
}

int sblas_hip_krylov_dot_f64(int dev, void *stream, int64_t n, int ndots, const double *const *x, const double *const *y, double *out,
                             void *workspace, size_t workspace_bytes)
{
    if (n < 0 || n > INT_MAX || ndots < 1 || ndots > KRYLOV_MAX_DOTS || !x || !y || !out) return SBLAS_E_INVALID;
    for (int q = 0; q < ndots; ++q)
        if (n > 0 && (!x[q] || !y[q])) return SBLAS_E_INVALID;
    if (!workspace || workspace_bytes < sblas_hip_krylov_dot_workspace(n, ndots)) return SBLAS_E_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 7u) return SBLAS_E_INVALID;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    hipStream_t s = (hipStream_t)stream;
    DotArgs a{n, krylov_cells(n), {}, {}, static_cast<double *>(workspace)};
    for (int q = 0; q < ndots; ++q) a.x[q] = x[q], a.y[q] = y[q];
    if (a.cells > 0) launch_dot(s, ndots, a);
    launch_fold(s, FOLD_OUT, ndots, 0, a.cells, a.part, out);
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_krylov_update_f64(int dev, void *stream, int op, int jacobi, int64_t n, const double *scalars, double *const *v, int nv,
                                double *partial)
{
    static const int need[5] = {4, 2, 3, 3, 7}, parts[5] = {1, 0, 0, 0, 2};
    if (op < SBLAS_KRYLOV_UP_PCG_XR || op > SBLAS_KRYLOV_UP_BICG_XR || n < 0 || n > INT_MAX || !scalars || !v) return SBLAS_E_INVALID;
    const bool jac = jacobi != 0 && op != SBLAS_KRYLOV_UP_PCG_P && op != SBLAS_KRYLOV_UP_BICG_XR;
    const int want = need[op] + (jac ? 2 : 0);
    if (nv < want || nv > 8) return SBLAS_E_INVALID;
    if (n == 0) return SBLAS_OK;
    for (int q = 0; q < want; ++q)
        if (!v[q]) return SBLAS_E_INVALID;
    if (parts[op] && !partial) return SBLAS_E_INVALID;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    UpArgs a{n, krylov_cells(n), const_cast<double *>(scalars), partial, {}};
    for (int q = 0; q < want; ++q) a.v[q] = v[q];
    launch_update((hipStream_t)stream, op, jac, a);
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_krylov_plan_create(int dev, void *stream, int method, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                                 const void *spmv_plan, int precond, const void *lower_plan, const void *upper_plan, void **plan_out)
{
    (void)stream; // nothing is copied: create is host work and one allocation
    if (!plan_out) return SBLAS_E_INVALID;
    *plan_out = nullptr;
    if (method != SBLAS_KRYLOV_PCG && method != SBLAS_KRYLOV_BICGSTAB) return SBLAS_E_INVALID;
    if (!precond_known(precond)) return SBLAS_E_INVALID;
    if (n < 0 || nnz < 0 || n > INT_MAX - 64 || nnz > INT_MAX) return SBLAS_E_INVALID;
    if (!rowptr || (nnz > 0 && !colidx) || (n == 0 && nnz != 0)) return SBLAS_E_INVALID;
    const int device = resolve_device(dev);
    if (spmv_plan && sblas_hip_spmv_plan_speaks_for(spmv_plan, device, n, n, nnz, rowptr, colidx) != SBLAS_OK) return SBLAS_E_INVALID;
    std::unique_ptr<KrylovPlan> p(new KrylovPlan);
    if (p->pre.bind(precond, lower_plan, upper_plan, device, n, nnz, rowptr, colidx) != SBLAS_OK) return SBLAS_E_INVALID;
    p->dev = device, p->method = method, p->n = n, p->nnz = nnz, p->cells = krylov_cells(n);
    p->rowptr = rowptr, p->colidx = colidx, p->spmv = spmv_plan;
    p->n_vectors = (method == SBLAS_KRYLOV_PCG ? KRYLOV_PCG_VECTORS : KRYLOV_BICGSTAB_VECTORS) + p->pre.applied();
    if (n == 0) {
        *plan_out = p.release();
        return SBLAS_OK;
    }
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    const size_t block_bytes = pad256(KRYLOV_BLOCK_SLOTS * 8);
    p->vector_bytes = pad256((size_t)n * 8);
    p->partial_bytes = pad256((size_t)KRYLOV_MAX_DOTS * (size_t)p->cells * 8);
    p->bytes = block_bytes + p->partial_bytes + (size_t)p->n_vectors * p->vector_bytes;
    if (p->buf.alloc(p->dev, p->bytes) != hipSuccess) return SBLAS_E_HIP;
    p->blk = p->buf.at<double>(), p->part = p->buf.at<double>(block_bytes), p->vec = p->buf.at<double>(block_bytes + p->partial_bytes);
    *plan_out = p.release();
    return SBLAS_OK;
}

int sblas_hip_krylov_plan_info(const void *plan, int64_t out[10])
{
    if (!plan || !out) return SBLAS_E_INVALID;
    const KrylovPlan *p = static_cast<const KrylovPlan *>(plan);
    int64_t lower[12], upper[12];
    p->pre.info(lower, upper);
    out[0] = p->n, out[1] = p->nnz, out[2] = p->method, out[3] = p->pre.kind, out[4] = p->n_vectors, out[5] = (int64_t)p->vector_bytes;
    out[6] = (int64_t)p->partial_bytes, out[7] = KRYLOV_BLOCK_SLOTS * 8, out[8] = (int64_t)p->bytes;
    out[9] = sblas_krylov_launches(p->method, p->pre.kind, lower, upper);
    return SBLAS_OK;
}

int sblas_hip_krylov_plan_destroy(void *plan)
{
    delete static_cast<KrylovPlan *>(plan);
    return SBLAS_OK;
}

int sblas_hip_krylov_start(void *plan, void *stream, const double *val, const double *lu_or_dinv, const double *b, double *x, double rtol,
                           double atol, int64_t max_iter)
{
    KrylovPlan *p = static_cast<KrylovPlan *>(plan);
    if (!p) return SBLAS_E_INVALID;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    if (!(rtol >= 0.0) || !(atol >= 0.0) || max_iter < 0) return SBLAS_E_INVALID; // a NaN tolerance is refused too
    p->started = false;
    if (p->n == 0) {
        p->started = true;
        return SBLAS_OK;
    }
    if (!b || !x || (p->nnz > 0 && !val) || !p->pre.take(lu_or_dinv)) return SBLAS_E_INVALID;
    p->val = val, p->x = x;
    hipStream_t s = (hipStream_t)stream;
    const bool pcg = p->method == SBLAS_KRYLOV_PCG, jac = p->pre.jacobi();
    int rc;
    dot(p, s, b, b);
    launch_fold(s, FOLD_START_B, 1, !pcg, p->cells, p->part, p->blk, rtol, atol, max_iter);
    double *bb = const_cast<double *>(b), *dinv = const_cast<double *>(p->pre.values);
    if (pcg) {
        double *r = p->w(V_R), *q = p->w(V_Q), *z = p->pre.none() ? r : p->w(V_Z);
        if ((rc = plan_spmv(p, s, x, q)) != SBLAS_OK) return rc;
        launch_update(s, UP_START_PCG, jac, up_args(p, {r, bb, q, dinv, z, x}));
        launch_fold(s, FOLD_START_R, jac ? 2 : 1, 0, p->cells, p->part, p->blk);
        if (p->pre.applied()) {
            if ((rc = p->pre.apply(s, r, p->w(V_TMP_PCG), z)) != SBLAS_OK) return rc;
            dot(p, s, r, z);
            launch_fold(s, FOLD_RHO0, 1, 0, p->cells, p->part, p->blk);
        }
        launch_update(s, UP_COPY, false, up_args(p, {p->w(V_P), z}));
    } else {
        double *v = p->w(B_V);
        if ((rc = plan_spmv(p, s, x, v)) != SBLAS_OK) return rc;
        launch_update(s, UP_START_BICG, false, up_args(p, {p->w(B_R), bb, v, p->w(B_RHAT), p->w(B_P), x}));
        launch_fold(s, FOLD_START_R, 1, 0, p->cells, p->part, p->blk);
    }
    if (hipGetLastError() != hipSuccess) return SBLAS_E_HIP;
    p->started = true;
    return SBLAS_OK;
}

int sblas_hip_krylov_iterate(void *plan, void *stream, int64_t k)
{
    const KrylovPlan *p = static_cast<const KrylovPlan *>(plan);
    if (!p || k < 0 || !p->started) return SBLAS_E_INVALID;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    if (p->n == 0) return SBLAS_OK;
    hipStream_t s = (hipStream_t)stream;
    for (int64_t it = 0; it < k; ++it) {
        const int rc = p->method == SBLAS_KRYLOV_PCG ? pcg_iteration(p, s) : bicgstab_iteration(p, s);
        if (rc != SBLAS_OK) return rc;
    }
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_krylov_status(const void *plan, void *stream, double out[8])
{
    const KrylovPlan *p = static_cast<const KrylovPlan *>(plan);
    if (!p || !out || !p->started) return SBLAS_E_INVALID;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    for (int q = 0; q < 8; ++q) out[q] = 0.0;
    if (p->n == 0) {
        out[0] = SBLAS_KRYLOV_CONVERGED;
        return SBLAS_OK;
    }
    double h[KRYLOV_BLOCK_SLOTS];
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(h, p->blk, sizeof h, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return SBLAS_E_HIP;
    long long ih[KRYLOV_BLOCK_SLOTS];
    memcpy(ih, h, sizeof ih);
    out[0] = (double)ih[KS_STATUS], out[1] = (double)ih[KS_ITER], out[2] = h[KS_RNORM], out[3] = h[KS_BNORM];
    out[4] = h[KS_ALPHA], out[5] = h[KS_BETA], out[6] = h[KS_OMEGA], out[7] = (double)ih[KS_WHICH];
    return SBLAS_OK;
}

} // extern "C"
