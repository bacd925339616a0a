// cheby.hip -- Chebyshev smoothing on a device eigenvalue estimate: z = p(D^-1 A) D^-1 r for a square CSR
// matrix with fp64 values, int32 indices, strictly ascending rows and a stored diagonal, p the degree-d Chebyshev
// polynomial on [lambda_max / ratio, lambda_max], and lambda_max(D^-1 A) estimated on the device.
//
// create is host work, as the AMG plan does it: the structure check that names the first bad row and the rows packed into
// four-lane units as one wide level of a solve.  setup is device work only: one kernel writes dinv = 1 / a_ii, folds the
// row bound g and flags a bad diagonal; the estimate is k steps of Jacobi-preconditioned CG on A x = b0 (Lanczos in the
// D-inner product, x never formed) as a fixed batch of launches whose scalars live in the device block; one lane then
// takes the scalar routine of cheby.h -- the tridiagonal, its largest Ritz value by Sturm bisection, the interval and the
// coefficient table -- so apply needs no host value.  apply is `degree` launches of ONE row kernel:
//   step   t_i = dinv_i (b_i - s_i(x)), d_i = c1_k d_i + c2_k t_i, y_i = x_i + d_i, s_i the AMG sweep's row sum;
//   from a guess the first step leaves c1 d out; from zero it is elementwise (the row sums vanish);
//   the same kernel's PRODUCT mode is y = A x, the estimate's.
// Nothing waits across workgroups: no flag polling, no cooperative launch, no atomics in apply (setup's maximum and flag
// are integer atomics, the same in every order); the only synchronisation is the kernel boundary.  setup and apply
// allocate nothing and never synchronise.
//
// The freeze.  Once a scalar of the recurrence is not finite and > 0, or the last step's alpha is taken, the status word is
// STOPPED: every later kernel of the batch returns at entry and lane 0 of every fold changes nothing, so m, the alphas and
// the betas stay what they were, and the host never looks.
//
// Results contract: cheby_row() is the one expression of a row, sweep_row()'s of amg.hip with the polynomial's step behind
// the fold: the lane group's width G(p) depends on the stored length p alone, lane l takes the entries l, l + G, ... with
// one fused multiply-add each from +0, and the lanes fold by the butterfly of rowwise.h.  Dots are the Krylov plans' (a
// cell a workgroup, krylov_fold.h).  Everything else is rounded operation by operation: contraction is off.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <memory>
#include <vector>
#include "../../include/sblas_hip.h"
#define CHEBY_HD __host__ __device__
#include "cheby.h"
#include "cheby_launch.h"
#include "color.h"
#include "level_kernels.h"
#include "rowwise.h"
#include "unit_row.h"

#pragma clang fp contract(off) // file scope: a * b + c below is two roundings; the row sum calls the fused one by name

#include "krylov_fold.h" // group_fold, cell_walk, cell_store: the dots are the Krylov plans'

using namespace sblas;

namespace {

enum { MODE_PRODUCT = 0, MODE_FROM_GUESS = 1, MODE_STEP = 2 };
enum { FOLD_START = 0, FOLD_PQ = 1, FOLD_RZ = 2 };

// Row u.row of y (and of d).  Every lane of the wave calls this together (the butterfly moves data between lanes); `quad`
// is the lane's place in its unit.  x and y are distinct arrays: other rows gather x while this one writes y.  d is read
// and written by its own row's writer alone.  coef: (c1_k, c2_k) of this step, one uniform address.
template <int MODE>
__device__ __forceinline__ void cheby_row(const SweepUnit u, int quad, const int32_t *__restrict__ colidx, const double *__restrict__ val,
                                          const double *__restrict__ dinv, const double *__restrict__ coef, const double *__restrict__ b,
                                          const double *__restrict__ x, double *__restrict__ d, double *__restrict__ y)
{
    const int gs = sptrsv_group_shift((int64_t)u.end - u.beg);
    const int lane = 4 * u.q + quad; // the lane's place among the row's G lanes
    const bool writer = u.row >= 0 && lane == 0;
    // what the row's last step needs travels with its first entries instead of waiting behind the fold
    const bool poly = MODE != MODE_PRODUCT;
    const double bi = writer && poly ? b[u.row] : 0.0;
    const double xi = writer && poly ? x[u.row] : 0.0;
    const double wi = writer && poly ? dinv[u.row] : 0.0;
    const double di = writer && MODE == MODE_STEP ? d[u.row] : 0.0;
    const double c1 = MODE == MODE_STEP ? coef[0] : 0.0, c2 = poly ? coef[1] : 0.0;
    const double si = unit_row_sum(u.row >= 0, u.beg, u.end, lane, gs, colidx, val, x);
    if (writer) {
        if constexpr (MODE == MODE_PRODUCT) {
            y[u.row] = si;
        } else {
            const double res = bi - si;
            const double t = wi * res;
            double dn = c2 * t;
            if constexpr (MODE == MODE_STEP) {
                const double kept = c1 * di;
                dn = kept + dn;
            }
            d[u.row] = dn;
            y[u.row] = xi + dn;
        }
    }
}

// status: the estimate's word (PRODUCT only): anything but RUNNING and the launch returns at entry, block-uniform
template <int MODE>
__global__ __launch_bounds__(CHEBY_THREADS) void cheby_step_kernel(int64_t count, const SweepUnit *__restrict__ units, const int32_t *__restrict__ colidx,
                                                                   const double *__restrict__ val, const double *__restrict__ dinv,
                                                                   const double *__restrict__ coef, const long long *__restrict__ status,
                                                                   const double *__restrict__ b, const double *__restrict__ x,
                                                                   double *__restrict__ d, double *__restrict__ y)
{
    if constexpr (MODE == MODE_PRODUCT)
        if (status[CS_STATUS] != CHEBY_RUNNING) return;
    cheby_row<MODE>(wide_unit<CHEBY_THREADS>(0, count, units, NO_SWEEP_UNIT), threadIdx.x & 3, colidx, val, dinv, coef, b, x, d, y);
}

// step 0 from a zero guess: the row sums vanish, d_i = c2_0 (dinv_i b_i) and x_i = d_i
__global__ __launch_bounds__(CHEBY_THREADS) void cheby_first_kernel(int64_t n, const double *__restrict__ dinv, const double *__restrict__ coef,
                                                                    const double *__restrict__ b, double *__restrict__ d, double *__restrict__ y)
{
    const int64_t i = (int64_t)blockIdx.x * CHEBY_THREADS + threadIdx.x;
    if (i >= n) return;
    const double t = dinv[i] * b[i];
    const double dn = coef[1] * t;
    d[i] = dn, y[i] = dn;
}

// dinv_i = 1 / a_ii; the row bound sum_e |a_ie| / a_ii (sequentially in stored order from +0, one rounded division) into
// the maximum g; a diagonal that is not finite and > 0 into the flag, the least (level, row).  Both by integer atomics, the same in
// every order: positive doubles order as their bit patterns do, and a bound that is not > 0 (a NaN too) is never the
// maximum.  A wave folds its maximum first, so that at most one lane in 64 reaches the slot.
__global__ __launch_bounds__(CHEBY_THREADS) void cheby_dinv_kernel(int64_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ dpos,
                                                                   const double *__restrict__ val, double *__restrict__ dinv, double *blk,
                                                                   unsigned long long *flag, int level)
{
    const int64_t i = (int64_t)blockIdx.x * CHEBY_THREADS + threadIdx.x;
    double most = 0.0;
    if (i < n) {
        const double d = val[dpos[i]];
        double s = 0.0;
        for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) s = s + fabs(val[e]);
        dinv[i] = 1.0 / d;
        const double bound = s / d;
        if (bound > 0.0) most = bound;
        if (!cheby_positive(d)) atomicMin(flag, ((unsigned long long)level << 32) | (unsigned long long)i);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const double other = __shfl_xor(most, m);
        if (other > most) most = other;
    }
    // the slot only grows, so a wave whose maximum does not exceed what it reads there (however stale) has nothing to add:
    // on a matrix whose rows share their bound, a few waves reach the slot instead of all of them in turn
    unsigned long long *slot = reinterpret_cast<unsigned long long *>(blk + CS_G);
    const unsigned long long mine = (unsigned long long)__double_as_longlong(most);
    if ((threadIdx.x & 63) == 0 && most > 0.0 && mine > *reinterpret_cast<volatile unsigned long long *>(slot)) atomicMax(slot, mine);
}

// ---- the estimate's vector passes: a cell a workgroup, as the Krylov plans' updates ------------------------------------
struct EstArgs {
    int64_t n, cells;
    double *blk, *part;
    const double *dinv;
    double *r, *z, *p, *q;
    uint32_t salt;
};

__device__ __forceinline__ bool stopped(const double *blk) { return reinterpret_cast<const long long *>(blk)[CS_STATUS] != CHEBY_RUNNING; }

// r = b0, z = dinv o r, p = z, and stage 1 of (r, z)
__global__ __launch_bounds__(KRYLOV_LANES) void cheby_start_kernel(const EstArgs a)
{
    double acc[1] = {};
    cell_walk(a.n, [&](int64_t i) {
        const double ri = cheby_start_value(color_priority((uint32_t)i, a.salt));
        const double zi = a.dinv[i] * ri;
        a.r[i] = ri, a.z[i] = zi, a.p[i] = zi;
        acc[0] = acc[0] + ri * zi;
    });
    cell_store<1>(acc, a.part, a.cells);
}

// stage 1 of (p, q)
__global__ __launch_bounds__(KRYLOV_LANES) void cheby_dot_kernel(const EstArgs a)
{
    if (stopped(a.blk)) return; // block-uniform, read once: the freeze
    double acc[1] = {};
    cell_walk(a.n, [&](int64_t i) { acc[0] = acc[0] + a.p[i] * a.q[i]; });
    cell_store<1>(acc, a.part, a.cells);
}

// r = r - alpha q, z = dinv o r, and stage 1 of (r, z)
__global__ __launch_bounds__(KRYLOV_LANES) void cheby_r_kernel(const EstArgs a)
{
    if (stopped(a.blk)) return;
    const double al = a.blk[CS_ALPHA];
    double acc[1] = {};
    cell_walk(a.n, [&](int64_t i) {
        const double ri = a.r[i] - al * a.q[i];
        const double zi = a.dinv[i] * ri;
        a.r[i] = ri, a.z[i] = zi;
        acc[0] = acc[0] + ri * zi;
    });
    cell_store<1>(acc, a.part, a.cells);
}

// p = z + beta p
__global__ __launch_bounds__(KRYLOV_LANES) void cheby_p_kernel(const EstArgs a)
{
    if (stopped(a.blk)) return;
    const double be = a.blk[CS_BETA];
    cell_walk(a.n, [&](int64_t i) { a.p[i] = a.z[i] + be * a.p[i]; });
}

// stage 2 of a dot, which is also the scalar step: ONE workgroup folds the cells' sums (lane t adds partial[t],
// partial[t + 256], ... in order from +0, then the butterfly) and its lane 0 takes the step that follows from them
__global__ __launch_bounds__(KRYLOV_LANES) void cheby_fold_kernel(int op, int j, int last, int64_t cells, const double *part, double *blk)
{
    double acc[1] = {}, d[1];
    for (int64_t c = threadIdx.x; c < cells; c += KRYLOV_LANES) acc[0] = acc[0] + part[c];
    group_fold<1>(acc, d);
    if (threadIdx.x != 0) return;
    long long *ib = reinterpret_cast<long long *>(blk);
    if (op == FOLD_START) { // every slot by its own type
        blk[CS_RHO] = d[0], blk[CS_ALPHA] = 0.0, blk[CS_BETA] = 0.0;
        ib[CS_M] = 0, ib[CS_STATUS] = CHEBY_RUNNING;
        return;
    }
    if (ib[CS_STATUS] != CHEBY_RUNNING) return; // frozen: the scalars stay what they were
    if (op == FOLD_PQ) {
        const double alpha = blk[CS_RHO] / d[0];
        if (!cheby_positive(d[0]) || !cheby_positive(alpha)) {
            ib[CS_STATUS] = CHEBY_STOPPED;
            return;
        }
        blk[CS_ALPHA] = alpha, blk[CS_ALPHAS + j] = alpha;
        ib[CS_M] = j + 1;
        if (last) ib[CS_STATUS] = CHEBY_STOPPED;
    } else {
        const double beta = d[0] / blk[CS_RHO];
        if (!cheby_positive(beta)) { // this beta is dropped
            ib[CS_STATUS] = CHEBY_STOPPED;
            return;
        }
        blk[CS_BETA] = beta, blk[CS_BETAS + j] = beta, blk[CS_RHO] = d[0];
    }
}

// one lane: the scalar routine of cheby.h on the block.  estimated = 0: lambda_max is the caller's and no step counts.
__global__ void cheby_finish_kernel(double *blk, int estimated, double boost, double ratio, double given, int degree)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    long long *ib = reinterpret_cast<long long *>(blk);
    if (!estimated) ib[CS_M] = 0;
    double out[3];
    cheby_finish(ib[CS_M], blk + CS_ALPHAS, blk + CS_BETAS, blk[CS_G], boost, ratio, given, degree, blk + CS_T, blk + CS_E2, out, blk + CS_TABLE);
    blk[CS_RITZ] = out[0], blk[CS_LMAX] = out[1], blk[CS_LMIN] = out[2];
}

inline unsigned grid_of(int64_t threads) { return (unsigned)((threads + CHEBY_THREADS - 1) / CHEBY_THREADS); }

struct ChebyPlan {
    int dev = -1, degree = 0, steps = 0;
    int64_t n = 0, nnz = 0, units = 0, cells = 0;
    double boost = 0.0, ratio = 0.0;
    uint32_t seed = 0;
    const int32_t *rowptr = nullptr, *colidx = nullptr; // the caller's
    DeviceBuffer ibuf, dbuf;                            // units | dpos;  block | partials | dinv | d | w | p | q
    ChebyOperator op;                                   // the matrix, dinv, the block and the partials; val is setup's
    double *blk = nullptr, *d = nullptr, *w = nullptr, *pv = nullptr, *qv = nullptr;
    size_t bytes = 0;
    bool ready = false; // setup's
};

template <int MODE>
void launch_step(hipStream_t s, const ChebyOperator &op, int k, const double *b, const double *x, double *d, double *y)
{
    cheby_step_kernel<MODE><<<wide_grid(4 * op.units, CHEBY_THREADS), CHEBY_THREADS, 0, s>>>(
        op.units, static_cast<const SweepUnit *>(op.d_units), op.colidx, op.val, op.dinv, op.blk + CS_TABLE + 2 * k,
        reinterpret_cast<const long long *>(op.blk), b, x, d, y);
}

// steps 1 .. degree - 1 behind a first step that wrote buf[cur]; the last write lands in buf[1]
void launch_rest(hipStream_t s, const ChebyPlan &p, const double *b, double *const buf[2], int cur)
{
    for (int k = 1; k < p.degree; ++k) launch_step<MODE_STEP>(s, p.op, k, b, buf[cur], p.d, buf[cur ^ 1]), cur ^= 1;
}

bool overlap(const double *a, const double *b, int64_t n) { return a < b + n && b < a + n; }

// launches of a setup that estimates: dinv, start and its fold, six a step but three for the last, the scalar routine
inline int64_t setup_launches(int steps) { return 1 + 2 + 6 * (int64_t)(steps - 1) + 3 + 1; }

} // namespace

namespace sblas {

void cheby_setup_launches(hipStream_t s, const ChebyOperator &op, unsigned long long *flag, int level, uint32_t seed, int steps, double boost,
                          double ratio, double given, int degree, double *r, double *z, double *p, double *q)
{
    const bool estimate = given != given;
    (void)hipMemsetAsync(op.blk + CS_G, 0, 8, s);
    cheby_dinv_kernel<<<grid_of(op.n), CHEBY_THREADS, 0, s>>>(op.n, op.rowptr, op.dpos, op.val, op.dinv, op.blk, flag, level);
    if (estimate) {
        const int64_t ncells = krylov_cells(op.n);
        const EstArgs a{op.n, ncells, op.blk, op.part, op.dinv, r, z, p, q, color_salt(seed + (uint32_t)level)};
        const unsigned cells = (unsigned)ncells;
        cheby_start_kernel<<<cells, KRYLOV_LANES, 0, s>>>(a);
        cheby_fold_kernel<<<1, KRYLOV_LANES, 0, s>>>(FOLD_START, 0, 0, ncells, op.part, op.blk);
        for (int j = 0; j < steps; ++j) {
            const bool last = j == steps - 1;
            launch_step<MODE_PRODUCT>(s, op, 0, nullptr, p, nullptr, q);
            cheby_dot_kernel<<<cells, KRYLOV_LANES, 0, s>>>(a);
            cheby_fold_kernel<<<1, KRYLOV_LANES, 0, s>>>(FOLD_PQ, j, last, ncells, op.part, op.blk);
            if (last) break;
            cheby_r_kernel<<<cells, KRYLOV_LANES, 0, s>>>(a);
            cheby_fold_kernel<<<1, KRYLOV_LANES, 0, s>>>(FOLD_RZ, j, 0, ncells, op.part, op.blk);
            cheby_p_kernel<<<cells, KRYLOV_LANES, 0, s>>>(a);
        }
    }
    cheby_finish_kernel<<<1, 64, 0, s>>>(op.blk, estimate, boost, ratio, given, degree);
}

void cheby_first_launch(hipStream_t s, const ChebyOperator &op, const double *b, double *d, double *y)
{
    cheby_first_kernel<<<grid_of(op.n), CHEBY_THREADS, 0, s>>>(op.n, op.dinv, op.blk + CS_TABLE, b, d, y);
}

void cheby_guess_launch(hipStream_t s, const ChebyOperator &op, const double *b, const double *x, double *d, double *y)
{
    launch_step<MODE_FROM_GUESS>(s, op, 0, b, x, d, y);
}

void cheby_step_launch(hipStream_t s, const ChebyOperator &op, int k, const double *b, const double *x, double *d, double *y)
{
    launch_step<MODE_STEP>(s, op, k, b, x, d, y);
}

} // namespace sblas

extern "C" {

int sblas_hip_cheby_plan_create(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx, int degree,
                                int eig_steps, double eig_boost, double eig_ratio, uint32_t seed, void **plan_out, int64_t *bad_row)
{
    if (bad_row) *bad_row = -1;
    if (!plan_out) return SBLAS_E_INVALID;
    *plan_out = nullptr;
    if (!cheby_degree_ok(degree) || !cheby_steps_ok(eig_steps) || !cheby_boost_ok(eig_boost) || !cheby_ratio_ok(eig_ratio)) return SBLAS_E_INVALID;
    if (n < 0 || nnz < 0 || n > INT_MAX - 64 || nnz > INT_MAX || (n == 0 && nnz != 0)) return SBLAS_E_INVALID;
    if ((n > 0 && !rowptr) || (nnz > 0 && !colidx)) return SBLAS_E_INVALID;
    std::unique_ptr<ChebyPlan> p(new ChebyPlan);
    p->dev = resolve_device(dev), p->degree = degree, p->steps = eig_steps, p->boost = eig_boost, p->ratio = eig_ratio, p->seed = seed;
    p->n = n, p->nnz = nnz, p->rowptr = rowptr, p->colidx = colidx, p->cells = krylov_cells(n);
    if (n == 0) {
        *plan_out = p.release();
        return SBLAS_OK;
    }
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int32_t> h_rowptr, h_colidx, dpos((size_t)n);
    int rc = fetch_structure(s, n, nnz, rowptr, colidx, h_rowptr, h_colidx, bad_row);
    if (rc != SBLAS_OK) return rc;
    int64_t bad = -1;
    rc = sblas_ilu0_check(n, h_rowptr.data(), h_colidx.data(), dpos.data(), &bad);
    if (rc != SBLAS_OK) {
        if (bad_row) *bad_row = bad;
        return rc;
    }
    // the rows packed as one wide level of a solve, as the AMG sweep's launch packs them
    std::vector<int32_t> zero_level((size_t)n, 0);
    LevelOrder o;
    std::vector<SweepUnit> units;
    const auto unit_of = [&](int32_t i, int32_t q) { return SweepUnit{i, h_rowptr[(size_t)i], h_rowptr[(size_t)i + 1], q}; };
    level_pack(n, h_rowptr.data(), zero_level.data(), 1, unit_of, NO_SWEEP_UNIT, o, units);
    p->units = p->op.units = (int64_t)units.size();
    Segment seg[2] = {Segment(units), Segment(dpos)};
    size_t ib = 0;
    if (upload_segments(p->ibuf, p->dev, s, seg, 2, &ib) != hipSuccess) return SBLAS_E_HIP;
    p->op.n = n, p->op.rowptr = rowptr, p->op.colidx = colidx;
    p->op.d_units = p->ibuf.at<SweepUnit>(), p->op.dpos = p->ibuf.at<int32_t>(seg[1].offset);
    const size_t block = pad256((size_t)CHEBY_BLOCK_SLOTS * 8), part = pad256((size_t)p->cells * 8), vec = pad256((size_t)n * 8);
    const size_t db = block + part + 5 * vec;
    if (p->dbuf.alloc(p->dev, db) != hipSuccess) return SBLAS_E_HIP;
    p->blk = p->op.blk = p->dbuf.at<double>(), p->op.part = p->dbuf.at<double>(block);
    double *v = p->dbuf.at<double>(block + part);
    const size_t stride = vec / 8;
    p->op.dinv = v, p->d = v + stride, p->w = v + 2 * stride, p->pv = v + 3 * stride, p->qv = v + 4 * stride;
    p->bytes = ib + db;
    if (hipMemsetAsync(p->blk, 0, block, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return SBLAS_E_HIP;
    *plan_out = p.release();
    return SBLAS_OK;
}

int sblas_hip_cheby_plan_info(const void *plan, int64_t out[12])
{
    if (!plan || !out) return SBLAS_E_INVALID;
    const ChebyPlan *p = static_cast<const ChebyPlan *>(plan);
    out[0] = p->n, out[1] = p->nnz, out[2] = p->degree, out[3] = p->steps, out[4] = p->units, out[5] = p->degree, out[6] = (int64_t)p->bytes;
    out[7] = p->ready, out[8] = setup_launches(p->steps), out[9] = p->seed, out[10] = out[11] = 0;
    return SBLAS_OK;
}

int sblas_hip_cheby_plan_speaks_for(const void *plan, int dev, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx)
{
    const ChebyPlan *p = static_cast<const ChebyPlan *>(plan);
    if (!p || p->dev != resolve_device(dev)) return SBLAS_E_INVALID;
    return n == p->n && nnz == p->nnz && rowptr == p->rowptr && colidx == p->colidx ? SBLAS_OK : SBLAS_E_INVALID;
}

int sblas_hip_cheby_plan_destroy(void *plan)
{
    delete static_cast<ChebyPlan *>(plan);
    return SBLAS_OK;
}

int sblas_hip_cheby_plan_setup(void *plan, void *stream, const double *val, double lambda_max)
{
    ChebyPlan *p = static_cast<ChebyPlan *>(plan);
    if (!p) return SBLAS_E_INVALID;
    const bool estimate = lambda_max != lambda_max;
    if (!estimate && !cheby_lambda_ok(lambda_max)) return SBLAS_E_INVALID;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    if (p->n > 0 && !val) return SBLAS_E_INVALID;
    p->ready = false;
    if (p->n == 0) {
        p->ready = true;
        return SBLAS_OK;
    }
    hipStream_t s = (hipStream_t)stream;
    p->op.val = val;
    if (hipMemsetAsync(p->blk + CS_FLAG, 0xff, 8, s) != hipSuccess) return SBLAS_E_HIP;
    // r and z live in the polynomial's d and w: no apply runs between a setup's launches
    cheby_setup_launches(s, p->op, reinterpret_cast<unsigned long long *>(p->blk + CS_FLAG), 0, p->seed, p->steps, p->boost, p->ratio, lambda_max,
                         p->degree, p->d, p->w, p->pv, p->qv);
    if (hipGetLastError() != hipSuccess) return SBLAS_E_HIP;
    p->ready = true;
    return SBLAS_OK;
}

int sblas_hip_cheby_plan_apply(const void *plan, void *stream, const double *r, double *z)
{
    const ChebyPlan *p = static_cast<const ChebyPlan *>(plan);
    if (!p || !p->ready) return SBLAS_E_INVALID;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    if (p->n == 0) return SBLAS_OK;
    if (!r || !z || overlap(r, z, p->n)) return SBLAS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    double *const buf[2] = {p->w, z};
    const int cur = cheby_first_buffer(p->degree);
    cheby_first_launch(s, p->op, r, p->d, buf[cur]);
    launch_rest(s, *p, r, buf, cur);
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_cheby_plan_smooth(const void *plan, void *stream, const double *b, const double *x, double *y)
{
    const ChebyPlan *p = static_cast<const ChebyPlan *>(plan);
    if (!p || !p->ready) return SBLAS_E_INVALID;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    if (p->n == 0) return SBLAS_OK;
    if (!b || !x || !y || overlap(b, y, p->n) || overlap(x, y, p->n)) return SBLAS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    double *const buf[2] = {p->w, y};
    const int cur = cheby_first_buffer(p->degree);
    cheby_guess_launch(s, p->op, b, x, p->d, buf[cur]);
    launch_rest(s, *p, b, buf, cur);
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_cheby_plan_check(const void *plan, void *stream, double out[6])
{
    const ChebyPlan *p = static_cast<const ChebyPlan *>(plan);
    if (!p || !out || !p->ready) return SBLAS_E_INVALID;
    out[0] = -1.0, out[1] = out[2] = out[3] = out[4] = out[5] = 0.0;
    if (p->n == 0) return SBLAS_OK;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    double h[CS_ALPHAS];
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(h, p->blk, sizeof h, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return SBLAS_E_HIP;
    long long ih[CS_ALPHAS];
    memcpy(ih, h, sizeof ih);
    if ((unsigned long long)ih[CS_FLAG] != ~0ull) out[0] = (double)ih[CS_FLAG];
    out[1] = (double)ih[CS_M], out[2] = h[CS_RITZ], out[3] = h[CS_G], out[4] = h[CS_LMAX], out[5] = h[CS_LMIN];
    return SBLAS_OK;
}

int sblas_hip_cheby_plan_scalars(const void *plan, void *stream, double *alpha, double *beta, double *table)
{
    const ChebyPlan *p = static_cast<const ChebyPlan *>(plan);
    if (!p || !p->ready) return SBLAS_E_INVALID;
    if (p->n == 0) return SBLAS_OK;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    if (alpha) e = hipMemcpyAsync(alpha, p->blk + CS_ALPHAS, CHEBY_MAX_STEPS * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && beta) e = hipMemcpyAsync(beta, p->blk + CS_BETAS, CHEBY_MAX_STEPS * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && table) e = hipMemcpyAsync(table, p->blk + CS_TABLE, (size_t)p->degree * 16, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

} // extern "C"
