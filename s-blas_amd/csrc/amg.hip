// amg.hip -- plain (unsmoothed) aggregation AMG on a device plan: z = M^-1 r by one V(nu, nu) cycle from
// a zero guess, for a square CSR matrix with fp64 values, int32 indices, strictly ascending rows and a stored diagonal.
//
// create is host work, as the level plans do it: every level is aggregated on the host by the pinned rule of
// amg_rule.cpp, and the coarse pattern of a level is the COO plan (dup = sum) of the triplets (agg[row], agg[col]) in
// stored order, sorted once on the device.  setup is device work only: a level's values are the COO plan's re-assembly of
// the level above (duplicates added left to right in input order) and one kernel writes the smoother's wd = omega / d.
// apply is a fixed sequence of launches of four kernels, the walk of amg.h:
//   sweep     y_i = x_i + wd_i (b_i - s_i), or the residual b_i - s_i, s_i the row sum in the solves' pinned order;
//   first     y_i = wd_i b_i, the first sweep from a zero guess;
//   restrict  b_c[I] = the sum of the residual over aggregate I's members, ascending, by one thread;
//   prolong   x_i = x_i + scale * e[agg[i]].
// Nothing waits across workgroups: no flag polling, no cooperative launch, no atomics in apply; the only synchronisation
// is the kernel boundary.  apply allocates nothing and never synchronises.
//
// Results contract: sweep_row() is the one expression of a row.  Its bits are a function of the row's stored entries in
// stored order, the x values they name, b_i, x_i and wd_i: the lane group's width G(p) depends on the stored length p
// alone, lane l takes the entries l, l + G, ... with one fused multiply-add each from +0, and the lanes fold by the
// butterfly of rowwise.h -- exactly the triangular solves' row sum (sptrsv.hip) over the whole row.  The rows are packed
// into waves as a solve's wide level packs them (level_plan.h with one level): which rows share a wave does not enter
// any row's sum.  Everything else is rounded operation by operation: this file is compiled with contraction off.
//
// Smoothed aggregation (sblas_hip_amg_plan_create_ex with SBLAS_AMG_SMOOTHED) keeps all of the above and
// replaces a level's transfers.  The tentative aggregates are the same rule's.  P_l's pattern is the COO plan (dup = sum) of
// the triplets (row(e), agg[col(e)]) in A_l's stored order; its values are that plan's re-assembly of t, where q_i =
// omega_P / a_ii (a rounded division), t_e = -(q_i a_ie) off the diagonal and 1 - q_i a_ii on it (a rounded product, then
// a rounded difference).  omega_P defaults to 2/3 = 4 / (3 rho) with rho(D^-1 A) taken as 2: no eigenvalue estimate; A is
// used unfiltered.  R_l = P_l^T by the device transpose (stable), its values gathered; A_{l+1} = R_l (A_l P_l) by two
// SpGEMM plans.  Both transfers of a cycle are transfer_row(): the sweep's row sum over a stored row of R_l (restrict:
// b_{l+1}[I] = s_I) or P_l (prolong: x_i = x_i + scale s_i, in place: only the coarse vector is gathered).  A level is
// kept only when amg_keep_level() says so (the coarsening guard, min_reduction), decided right after the aggregation.
//
// Aggregation on the device (sblas_hip_amg_plan_create_dev with SBLAS_AMG_AGG_DEVICE) builds the same
// plan, array for array, without the host rule: every level is aggregated by sblas_hip_amg_aggregate_i32
// (amg_aggregate.hip) on the level's device arrays, one kernel writes the triplets from agg (a thread an entry), with
// theta > 0 the next level's values are the COO plan's assembly on the device (the same left-to-right sums), and below
// level 0 dpos comes from a kernel: only level 0's structure (for the check that names the first bad row), every level's
// row pointer (level_pack) and scalars come to the host.
//
// The Chebyshev smoother (sblas_hip_amg_plan_setup_ex with SBLAS_AMG_CHEBYSHEV) keeps all of the above and
// replaces a level's smoothings: the walk of amg.h takes a polynomial of `degree` launches where it takes a sweep, the
// launches are cheby.hip's (cheby_launch.h: one ChebyOperator a level, wd as its dinv), and setup runs a level's eigenvalue
// estimate where it ran the level's wd kernel.  Its buffers are made by a plan's first such setup, never by any other.
//
// The block cycle (sblas_hip_amg_plan_apply_multi) is the same walk on n x s row-major blocks: a second
// Ops of amg_cycle whose launches are amg_multi_kernels.h's: sweep_row() and transfer_row() eight columns abreast.
// Column j of its result has the bits of apply() on column j.  Its level vectors are made by sblas_hip_amg_plan_reserve_multi,
// never by any other call; a plan that never reserves keeps its bytes.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <memory>
#include <vector>
#include "../../include/sblas_hip.h"
#include "amg.h"
#include "amg_multi.h"
#include "cheby.h"
#include "cheby_launch.h"
#include "krylov.h"
#include "level_kernels.h"
#include "rowwise.h"
#include "unit_row.h"

#pragma clang fp contract(off) // file scope: a * b + c below is two roundings; the row sum calls the fused one by name

using namespace sblas;

namespace {

constexpr unsigned long long FLAG_CLEAN = ~0ull;

enum { MODE_SWEEP = 0, MODE_RESIDUAL = 1, MODE_FIRST = 2 };

// Row u.row of y.  Every lane of the wave calls this together (the butterfly moves data between lanes); `quad` is the
// lane's place in its unit.  x and y are distinct arrays: other rows gather x while this one writes y.
template <int MODE>
__device__ __forceinline__ void sweep_row(const SweepUnit u, int quad, const int32_t *__restrict__ colidx, const double *__restrict__ val,
                                          const double *__restrict__ wd, const double *__restrict__ b, const double *__restrict__ x,
                                          double *__restrict__ y)
{
    const int gs = sptrsv_group_shift((int64_t)u.end - u.beg);
    const int lane = 4 * u.q + quad; // the lane's place among the row's G lanes
    const bool writer = u.row >= 0 && lane == 0;
    // what the row's last step needs travels with its first entries instead of waiting behind the fold
    const double bi = writer ? b[u.row] : 0.0;
    const double xi = writer && MODE == MODE_SWEEP ? x[u.row] : 0.0;
    const double wi = writer && MODE == MODE_SWEEP ? wd[u.row] : 0.0;
    const double si = unit_row_sum(u.row >= 0, u.beg, u.end, lane, gs, colidx, val, x);
    if (writer) {
        const double d = bi - si;
        if constexpr (MODE == MODE_RESIDUAL) {
            y[u.row] = d;
        } else {
            const double t = wi * d;
            y[u.row] = xi + t;
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(AMG_THREADS) void amg_sweep_kernel(int64_t count, const SweepUnit *__restrict__ units, const int32_t *__restrict__ colidx,
                                                                const double *__restrict__ val, const double *__restrict__ wd,
                                                                const double *__restrict__ b, const double *__restrict__ x,
                                                                double *__restrict__ y)
{
    sweep_row<MODE>(wide_unit<AMG_THREADS>(0, count, units, NO_SWEEP_UNIT), threadIdx.x & 3, colidx, val, wd, b, x, y);
}

// the first sweep from a zero guess: the row sums vanish, x_i + wd_i (b_i - 0) is wd_i b_i
__global__ __launch_bounds__(AMG_THREADS) void amg_first_kernel(int64_t n, const double *__restrict__ wd, const double *__restrict__ b,
                                                                double *__restrict__ y)
{
    const int64_t i = (int64_t)blockIdx.x * AMG_THREADS + threadIdx.x;
    if (i < n) y[i] = wd[i] * b[i];
}

// one thread an aggregate: its members ascending, sequentially from +0
__global__ __launch_bounds__(AMG_THREADS) void amg_restrict_kernel(int64_t n_agg, const int32_t *__restrict__ aggptr,
                                                                   const int32_t *__restrict__ members, const double *__restrict__ res,
                                                                   double *__restrict__ bc)
{
    const int64_t a = (int64_t)blockIdx.x * AMG_THREADS + threadIdx.x;
    if (a >= n_agg) return;
    double s = 0.0;
    for (int64_t k = aggptr[a]; k < aggptr[a + 1]; ++k) s = s + res[members[k]];
    bc[a] = s;
}

__global__ __launch_bounds__(AMG_THREADS) void amg_prolong_kernel(int64_t n, const int32_t *__restrict__ agg, double scale,
                                                                  const double *__restrict__ e, double *__restrict__ x)
{
    const int64_t i = (int64_t)blockIdx.x * AMG_THREADS + threadIdx.x;
    if (i >= n) return;
    const double t = scale * e[agg[i]];
    x[i] = x[i] + t;
}

// Row u.row of a transfer operator M (R_l or P_l) times `in`, sweep_row's row sum.  Every lane of the wave calls this
// together.  `out` is never gathered: the prolongation updates it in place.
template <int MODE>
__device__ __forceinline__ void transfer_row(const SweepUnit u, int quad, const int32_t *__restrict__ colidx, const double *__restrict__ val,
                                             double scale, const double *__restrict__ in, double *__restrict__ out)
{
    const int gs = sptrsv_group_shift((int64_t)u.end - u.beg);
    const int lane = 4 * u.q + quad;
    const bool writer = u.row >= 0 && lane == 0;
    const double xi = writer && MODE == AMG_PROLONG ? out[u.row] : 0.0; // travels with the first entries, as in sweep_row
    const double si = unit_row_sum(u.row >= 0, u.beg, u.end, lane, gs, colidx, val, in);
    if (writer) {
        if constexpr (MODE == AMG_RESTRICT) {
            out[u.row] = si;
        } else {
            const double t = scale * si;
            out[u.row] = xi + t;
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(AMG_THREADS) void amg_transfer_kernel(int64_t count, const SweepUnit *__restrict__ units,
                                                                   const int32_t *__restrict__ colidx, const double *__restrict__ val, double scale,
                                                                   const double *__restrict__ in, double *__restrict__ out)
{
    transfer_row<MODE>(wide_unit<AMG_THREADS>(0, count, units, NO_SWEEP_UNIT), threadIdx.x & 3, colidx, val, scale, in, out);
}

// t for every stored entry of A_l, over the sweep's units: the row's G(p) lanes take the entries l, l + G, ...; every lane
// forms q_i itself (one address a row).  No lane talks to another, so a pad's lanes leave at once.
__global__ __launch_bounds__(AMG_THREADS) void amg_pvalues_kernel(int64_t count, const SweepUnit *__restrict__ units, const int32_t *__restrict__ dpos,
                                                                  const double *__restrict__ val, double omega_p, double *__restrict__ t)
{
    const SweepUnit u = wide_unit<AMG_THREADS>(0, count, units, NO_SWEEP_UNIT);
    if (u.row < 0) return;
    const int G = 1 << sptrsv_group_shift((int64_t)u.end - u.beg);
    const int lane = 4 * u.q + (threadIdx.x & 3);
    const int64_t dp = dpos[u.row];
    const double q = omega_p / val[dp];
    for (int64_t e = (int64_t)u.beg + lane; e < u.end; e += G) {
        const double prod = q * val[e];
        t[e] = e == dp ? 1.0 - prod : -prod;
    }
}

// The triplets of a level's COO plan from agg, a thread an entry: entry e of row i is (agg[i], agg[col(e)]) for the plain
// plan's coarse pattern (COARSE_ROWS) and (i, agg[col(e)]) for P.  The row of e by bisection of rowptr, as the
// permutation plan's relabel kernel finds it.
template <bool COARSE_ROWS>
__global__ __launch_bounds__(AMG_THREADS) void amg_triplets_kernel(int64_t nnz, int64_t n, const int32_t *__restrict__ rowptr,
                                                                   const int32_t *__restrict__ colidx, const int32_t *__restrict__ agg,
                                                                   int32_t *__restrict__ trow, int32_t *__restrict__ tcol)
{
    const int64_t e = (int64_t)blockIdx.x * AMG_THREADS + threadIdx.x;
    if (e >= nnz) return;
    int64_t lo = 0, hi = n - 1; // the last row whose start is <= e (empty rows share their start with the next)
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (rowptr[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    trow[e] = COARSE_ROWS ? agg[lo] : (int32_t)lo;
    tcol[e] = agg[colidx[e]];
}

// dpos[i] = the place of the diagonal in the strictly ascending row i, by bisection.  A level below the first always
// stores it: row I of a coarse pattern holds the image of a member's diagonal entry.
__global__ __launch_bounds__(AMG_THREADS) void amg_dpos_kernel(int64_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                                                               int32_t *__restrict__ dpos)
{
    const int64_t i = (int64_t)blockIdx.x * AMG_THREADS + threadIdx.x;
    if (i >= n) return;
    int64_t lo = rowptr[i], hi = rowptr[i + 1]; // the first entry whose column is not below i
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)colidx[mid] < i) lo = mid + 1;
        else hi = mid;
    }
    dpos[i] = (int32_t)lo;
}

// wd_i = omega / a_ii (Jacobi) or omega / sum_e |a_ie| (l1, sequentially in stored order from +0).  A diagonal that is
// not finite and > 0 is reported as (level, row) in *flag: the least such pair, whichever thread finds it first -- an
// integer minimum is the same in every order.
__global__ __launch_bounds__(AMG_THREADS) void amg_wd_kernel(int64_t n, int level, int smoother, double omega, const int32_t *__restrict__ rowptr,
                                                             const int32_t *__restrict__ dpos, const double *__restrict__ val,
                                                             double *__restrict__ wd, unsigned long long *flag)
{
    const int64_t i = (int64_t)blockIdx.x * AMG_THREADS + threadIdx.x;
    if (i >= n) return;
    const double d = val[dpos[i]];
    double den = d;
    if (smoother == SBLAS_AMG_L1) {
        double s = 0.0;
        for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) s = s + fabs(val[e]);
        den = s;
    }
    wd[i] = omega / den;
    if (!(isfinite(d) && d > 0.0)) atomicMin(flag, ((unsigned long long)level << 32) | (unsigned long long)i);
}

inline unsigned grid_of(int64_t threads) { return (unsigned)((threads + AMG_THREADS - 1) / AMG_THREADS); }

} // namespace

#include "amg_multi_kernels.h" // the kernels above on a tile of columns: after the modes, the row functions and contract(off)

namespace {

struct AmgLevel {
    int64_t n = 0, nnz = 0, n_coarse = 0, units = 0;
    const int32_t *rowptr = nullptr, *colidx = nullptr; // level 0: the caller's; below: the COO plan's of the level above
    const double *val = nullptr;                        // level 0: setup's; below: own_val
    void *coo = nullptr;                                // the plan that makes level l + 1's structure and values
    DeviceBuffer ibuf, dbuf;                            // units | dpos | agg | aggptr | members;  wd | x0 | x1 | res | b | val
    SweepUnit *d_units = nullptr;
    int32_t *dpos = nullptr, *agg = nullptr, *aggptr = nullptr, *members = nullptr;
    double *wd = nullptr, *x[2] = {nullptr, nullptr}, *res = nullptr, *b = nullptr, *own_val = nullptr;
    size_t bytes = 0;
    // a smoothed level above the coarsest: `coo` makes P_l; R_l = P_l^T; ap = A_l P_l, rap = R_l ap = A_{l+1}
    void *ap = nullptr, *rap = nullptr;
    int64_t nnz_p = 0, nnz_ap = 0, p_units = 0, r_units = 0;
    const int32_t *p_rowptr = nullptr, *p_colidx = nullptr;                 // the COO plan's
    int32_t *r_rowptr = nullptr, *r_colidx = nullptr, *r_perm = nullptr; // tbuf: r_rowptr | r_colidx | r_perm | P's units | R's units
    SweepUnit *d_p_units = nullptr, *d_r_units = nullptr;
    double *p_val = nullptr, *r_val = nullptr, *ap_val = nullptr;           // tval: p_val | r_val | ap_val
    DeviceBuffer tbuf, ubuf, tval;
    // the Chebyshev smoother's, made by the plan's first such setup: d | the scalar block with the table | the dots' partials
    DeviceBuffer cbuf;
    double *d = nullptr;
    ChebyOperator cheb;
    size_t cheb_bytes = 0;
    // the block cycle's, made by reserve_multi alone: x0 | x1 | res | b of n x the reserved width
    DeviceBuffer mbuf;
    double *mx[2] = {nullptr, nullptr}, *mres = nullptr, *mb = nullptr;
    ~AmgLevel()
    {
        if (coo) sblas_hip_coo_plan_destroy(coo);
        if (ap) sblas_hip_spgemm_plan_destroy(ap);
        if (rap) sblas_hip_spgemm_plan_destroy(rap);
    }
};

struct AmgPlan {
    int dev = -1;
    int64_t n = 0, nnz = 0;
    const int32_t *rowptr = nullptr, *colidx = nullptr; // the caller's
    double theta = 0.0;
    uint32_t seed = 0;
    int prolongator = SBLAS_AMG_PLAIN, aggregation = SBLAS_AMG_AGG_HOST;
    double omega_p = 0.0, min_reduction = 0.0;
    std::vector<std::unique_ptr<AmgLevel>> lv;
    DeviceBuffer block, tscratch; // the flag word; a smoothed plan's t, sized by the level with the most entries
    double *t = nullptr;
    size_t t_bytes = 0;
    bool smoothed() const { return prolongator == SBLAS_AMG_SMOOTHED; }
    unsigned long long *flag = nullptr;
    // setup's
    bool ready = false;
    int smoother = SBLAS_AMG_JACOBI, nu = AMG_NU, coarse_sweeps = AMG_COARSE_SWEEPS;
    double omega = 0.0, scale = 1.0;
    // the Chebyshev smoother's: the estimate's four work vectors, sized by level 0 and shared by the levels (they run one
    // after the other), made with the levels' buffers by the first such setup
    DeviceBuffer ebuf;
    double *est[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t cheb_bytes = 0;
    int degree = 0; // of the last setup: 0 with the Jacobi and l1 sweeps
    int multi_width = 0; // the block cycle's reserved columns
    size_t multi_bytes = 0;
    int levels() const { return (int)lv.size(); }
};

void launch_sweep(hipStream_t s, const AmgLevel &L, int mode, const double *b, const double *x, double *y)
{
    if (mode == MODE_FIRST) amg_first_kernel<<<grid_of(L.n), AMG_THREADS, 0, s>>>(L.n, L.wd, b, y);
    else if (mode == MODE_RESIDUAL)
        amg_sweep_kernel<MODE_RESIDUAL><<<wide_grid(4 * L.units, AMG_THREADS), AMG_THREADS, 0, s>>>(L.units, L.d_units, L.colidx, L.val, L.wd, b, x, y);
    else
        amg_sweep_kernel<MODE_SWEEP><<<wide_grid(4 * L.units, AMG_THREADS), AMG_THREADS, 0, s>>>(L.units, L.d_units, L.colidx, L.val, L.wd, b, x, y);
}

void launch_restrict(hipStream_t s, const AmgPlan &p, const AmgLevel &L, const double *res, double *bc)
{
    if (p.smoothed())
        amg_transfer_kernel<AMG_RESTRICT><<<wide_grid(4 * L.r_units, AMG_THREADS), AMG_THREADS, 0, s>>>(L.r_units, L.d_r_units, L.r_colidx, L.r_val, 0.0, res, bc);
    else
        amg_restrict_kernel<<<grid_of(L.n_coarse), AMG_THREADS, 0, s>>>(L.n_coarse, L.aggptr, L.members, res, bc);
}

void launch_prolong(hipStream_t s, const AmgPlan &p, const AmgLevel &L, double scale, const double *e, double *x)
{
    if (p.smoothed())
        amg_transfer_kernel<AMG_PROLONG><<<wide_grid(4 * L.p_units, AMG_THREADS), AMG_THREADS, 0, s>>>(L.p_units, L.d_p_units, L.p_colidx, L.p_val, scale, e, x);
    else
        amg_prolong_kernel<<<grid_of(L.n), AMG_THREADS, 0, s>>>(L.n, L.agg, scale, e, x);
}

void launch_pvalues(hipStream_t s, const AmgLevel &L, double omega_p, const double *val, double *t)
{
    amg_pvalues_kernel<<<wide_grid(4 * L.units, AMG_THREADS), AMG_THREADS, 0, s>>>(L.units, L.d_units, L.dpos, val, omega_p, t);
}

// A smoothed level's numeric chain after its t: P's values, R's, A P and R (A P) into `coarse`.  Launches only.
int smoothed_values(hipStream_t s, const AmgPlan &p, const AmgLevel &L, const double *val, const double *t, double *coarse)
{
    int rc = sblas_hip_coo_plan_assemble(L.coo, s, t, L.p_val);
    if (rc == SBLAS_OK) rc = sblas_hip_gather_f64(p.dev, s, L.nnz_p, L.r_perm, L.p_val, L.r_val);
    if (rc == SBLAS_OK) rc = sblas_hip_spgemm_plan_numeric(L.ap, s, val, L.p_val, L.ap_val);
    if (rc == SBLAS_OK) rc = sblas_hip_spgemm_plan_numeric(L.rap, s, L.r_val, L.ap_val, coarse);
    return rc;
}

// the walk of amg.h as launches; level 0 reads the caller's r and ends in the caller's z
struct DeviceOps {
    const AmgPlan *p;
    hipStream_t s;
    const double *r;
    double *z;
    const double *b(int l) const { return l ? p->lv[(size_t)l]->b : r; }
    double *x(int l, int k) const { return l == 0 && k == AMG_RESULT_BUFFER ? z : p->lv[(size_t)l]->x[k]; }
    void first(int l, int dst) { launch_sweep(s, *p->lv[(size_t)l], MODE_FIRST, b(l), nullptr, x(l, dst)); }
    void sweep(int l, int src, int dst) { launch_sweep(s, *p->lv[(size_t)l], MODE_SWEEP, b(l), x(l, src), x(l, dst)); }
    void poly_first(int l, int dst) { cheby_first_launch(s, p->lv[(size_t)l]->cheb, b(l), p->lv[(size_t)l]->d, x(l, dst)); }
    void poly_guess(int l, int src, int dst) { cheby_guess_launch(s, p->lv[(size_t)l]->cheb, b(l), x(l, src), p->lv[(size_t)l]->d, x(l, dst)); }
    void poly_step(int l, int k, int src, int dst)
    {
        cheby_step_launch(s, p->lv[(size_t)l]->cheb, k, b(l), x(l, src), p->lv[(size_t)l]->d, x(l, dst));
    }
    void residual(int l, int src) { launch_sweep(s, *p->lv[(size_t)l], MODE_RESIDUAL, b(l), x(l, src), p->lv[(size_t)l]->res); }
    void restrict_to(int l)
    {
        const AmgLevel &L = *p->lv[(size_t)l];
        launch_restrict(s, *p, L, L.res, p->lv[(size_t)l + 1]->b);
    }
    void prolong(int l, int dst)
    {
        launch_prolong(s, *p, *p->lv[(size_t)l], p->scale, x(l + 1, AMG_RESULT_BUFFER), x(l, dst));
    }
};

bool overlap(const double *a, const double *b, int64_t n) { return a < b + n && b < a + n; }

// ---- the block cycle ---------------------------------------------------------------------------------------------------
// an n x s row-major block at leading dimension ld
struct Blk {
    const double *p;
    int64_t ld;
};

void launch_sweep_multi(hipStream_t st, const AmgLevel &L, int mode, int s, Blk b, Blk x, double *y, int64_t ldy)
{
    if (mode == MODE_FIRST) {
        amg_first_multi_kernel<<<grid_of(L.n * s), AMG_THREADS, 0, st>>>(L.n, s, L.wd, b.p, b.ld, y, ldy);
        return;
    }
    if (L.units == 0) return;
    const SweepMultiArgs a{L.units, unit_blocks(L.units, AMG_UNITS_PER_BLOCK), s, L.d_units, L.colidx, L.val, L.wd, b.p, x.p, y, b.ld, x.ld, ldy};
    if (mode == MODE_RESIDUAL) launch_sweep_multi_mode<MODE_RESIDUAL>(st, a);
    else launch_sweep_multi_mode<MODE_SWEEP>(st, a);
}

void launch_restrict_multi(hipStream_t st, const AmgPlan &p, const AmgLevel &L, int s, Blk res, double *bc, int64_t ldc)
{
    if (p.smoothed()) {
        if (L.r_units == 0) return;
        launch_transfer_multi_mode<AMG_RESTRICT>(
            st, TransferMultiArgs{L.r_units, unit_blocks(L.r_units, AMG_UNITS_PER_BLOCK), s, L.d_r_units, L.r_colidx, L.r_val, 0.0, res.p, bc, res.ld, ldc});
    } else {
        amg_restrict_multi_kernel<<<grid_of(L.n_coarse * s), AMG_THREADS, 0, st>>>(L.n_coarse, s, L.aggptr, L.members, res.p, res.ld, bc, ldc);
    }
}

void launch_prolong_multi(hipStream_t st, const AmgPlan &p, const AmgLevel &L, int s, double scale, Blk e, double *x, int64_t ldx)
{
    if (p.smoothed()) {
        if (L.p_units == 0) return;
        launch_transfer_multi_mode<AMG_PROLONG>(
            st, TransferMultiArgs{L.p_units, unit_blocks(L.p_units, AMG_UNITS_PER_BLOCK), s, L.d_p_units, L.p_colidx, L.p_val, scale, e.p, x, e.ld, ldx});
    } else {
        amg_prolong_multi_kernel<<<grid_of(L.n * s), AMG_THREADS, 0, st>>>(L.n, s, L.agg, scale, e.p, e.ld, x, ldx);
    }
}

// the walk of amg.h on blocks; level 0 reads the caller's R (ldr) and ends in the caller's Z (ldz), the level vectors
// inside the plan have leading dimension s.  The polynomial calls are never made: apply_multi passes degree 0.
struct MultiOps {
    const AmgPlan *p;
    hipStream_t st;
    int s;
    Blk r;
    double *z;
    int64_t ldz;
    const AmgLevel &lv(int l) const { return *p->lv[(size_t)l]; }
    Blk b(int l) const { return l ? Blk{lv(l).mb, s} : r; }
    double *x(int l, int k) const { return l == 0 && k == AMG_RESULT_BUFFER ? z : lv(l).mx[k]; }
    int64_t ldx(int l, int k) const { return l == 0 && k == AMG_RESULT_BUFFER ? ldz : s; }
    Blk xb(int l, int k) const { return Blk{x(l, k), ldx(l, k)}; }
    void first(int l, int dst) { launch_sweep_multi(st, lv(l), MODE_FIRST, s, b(l), Blk{nullptr, 0}, x(l, dst), ldx(l, dst)); }
    void sweep(int l, int src, int dst) { launch_sweep_multi(st, lv(l), MODE_SWEEP, s, b(l), xb(l, src), x(l, dst), ldx(l, dst)); }
    void poly_first(int, int) {}
    void poly_guess(int, int, int) {}
    void poly_step(int, int, int, int) {}
    void residual(int l, int src) { launch_sweep_multi(st, lv(l), MODE_RESIDUAL, s, b(l), xb(l, src), lv(l).mres, s); }
    void restrict_to(int l) { launch_restrict_multi(st, *p, lv(l), s, Blk{lv(l).mres, s}, lv(l + 1).mb, s); }
    void prolong(int l, int dst) { launch_prolong_multi(st, *p, lv(l), s, p->scale, xb(l + 1, AMG_RESULT_BUFFER), x(l, dst), ldx(l, dst)); }
};

inline size_t span_bytes(int64_t n, int s, int64_t ld) { return n > 0 ? ((size_t)(n - 1) * (size_t)ld + (size_t)s) * 8 : 0; }
// two n_a x s and n_b x s blocks overlap as address ranges
bool blocks_overlap(const double *a, int64_t na, int64_t lda, const double *b, int64_t nb, int64_t ldb, int s)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + span_bytes(nb, s, ldb) && b0 < a0 + span_bytes(na, s, lda);
}
// a block argument of a multi-column entry: present, 8-byte aligned, ld >= s
bool block_ok(const double *p, int64_t ld, int s) { return p && ld >= s && (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// every row kernel of the level at s columns fits a launch: false where tile_grid() refuses
bool multi_grids_ok(const AmgLevel &L, int s)
{
    for (const int64_t units : {L.units, L.r_units, L.p_units})
        if (tile_grid(unit_blocks(units, AMG_UNITS_PER_BLOCK), s) < 0) return false;
    return true;
}

// the plan's level `level` for a single-kernel entry, or null
const AmgLevel *level_of(const void *plan, int level, bool need_setup)
{
    const AmgPlan *p = static_cast<const AmgPlan *>(plan);
    if (!p || level < 0 || level >= p->levels() || (need_setup && !p->ready) || p->dev != resolve_device(-1)) return nullptr;
    return p->lv[(size_t)level].get();
}

// a level's row pointer alone on its way to the host (aggregation on the device: nothing nnz-sized follows it)
int fetch_rowptr(hipStream_t s, int64_t n, int64_t nnz, const int32_t *rowptr, std::vector<int32_t> &h_rowptr)
{
    h_rowptr.resize((size_t)n + 1);
    if (hipMemcpyAsync(h_rowptr.data(), rowptr, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return SBLAS_E_HIP;
    return h_rowptr[(size_t)n] == nnz ? SBLAS_OK : SBLAS_E_INTERNAL;
}

} // namespace

extern "C" {

int sblas_hip_amg_plan_create(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx, const double *val,
                              double theta, int64_t coarse_max, int max_levels, uint32_t seed, void **plan_out, int64_t *bad_row)
{
    return sblas_hip_amg_plan_create_ex(dev, stream, n, nnz, rowptr, colidx, val, theta, coarse_max, max_levels, seed, SBLAS_AMG_PLAIN, 0.0, 0.0,
                                        plan_out, bad_row);
}

int sblas_hip_amg_plan_create_ex(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx, const double *val,
                                 double theta, int64_t coarse_max, int max_levels, uint32_t seed, int prolongator, double prolong_omega,
                                 double min_reduction, void **plan_out, int64_t *bad_row)
{
    return sblas_hip_amg_plan_create_dev(dev, stream, n, nnz, rowptr, colidx, val, theta, coarse_max, max_levels, seed, prolongator, prolong_omega,
                                         min_reduction, SBLAS_AMG_AGG_HOST, plan_out, bad_row);
}

int sblas_hip_amg_plan_create_dev(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx, const double *val,
                                  double theta, int64_t coarse_max, int max_levels, uint32_t seed, int prolongator, double prolong_omega,
                                  double min_reduction, int aggregation, void **plan_out, int64_t *bad_row)
{
    if (bad_row) *bad_row = -1;
    if (!plan_out) return SBLAS_E_INVALID;
    *plan_out = nullptr;
    if (aggregation != SBLAS_AMG_AGG_HOST && aggregation != SBLAS_AMG_AGG_DEVICE) return SBLAS_E_INVALID;
    const bool dev_agg = aggregation == SBLAS_AMG_AGG_DEVICE;
    if (prolongator != SBLAS_AMG_PLAIN && prolongator != SBLAS_AMG_SMOOTHED) return SBLAS_E_INVALID;
    const bool smoothed = prolongator == SBLAS_AMG_SMOOTHED;
    if ((smoothed && !amg_prolong_omega_ok(prolong_omega)) || !amg_min_reduction_ok(min_reduction)) return SBLAS_E_INVALID;
    if (n < 0 || nnz < 0 || n > INT_MAX - 64 || nnz > INT_MAX || (n == 0 && nnz != 0)) return SBLAS_E_INVALID;
    if (!amg_theta_ok(theta) || (theta > 0.0 && !val)) return SBLAS_E_INVALID;
    if (coarse_max < 0 || max_levels < 0 || max_levels > AMG_LEVEL_CAP) return SBLAS_E_INVALID;
    if ((n > 0 && !rowptr) || (nnz > 0 && !colidx)) return SBLAS_E_INVALID;
    if (coarse_max == 0) coarse_max = AMG_COARSE_MAX;
    if (max_levels == 0) max_levels = AMG_MAX_LEVELS;
    std::unique_ptr<AmgPlan> p(new AmgPlan);
    p->dev = resolve_device(dev), p->n = n, p->nnz = nnz, p->rowptr = rowptr, p->colidx = colidx, p->theta = theta, p->seed = seed;
    p->prolongator = prolongator, p->omega_p = smoothed ? prolong_omega : 0.0, p->min_reduction = min_reduction, p->aggregation = aggregation;
    if (n == 0) {
        *plan_out = p.release();
        return SBLAS_OK;
    }
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int32_t> h_rowptr, h_colidx;
    std::vector<double> h_val;
    int rc = fetch_structure(s, n, nnz, rowptr, colidx, h_rowptr, h_colidx, bad_row);
    if (rc != SBLAS_OK) return rc;
    const bool by_value = theta > 0.0;
    if (by_value && !dev_agg) {
        h_val.resize((size_t)nnz);
        if (hipMemcpyAsync(h_val.data(), val, (size_t)nnz * 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            return SBLAS_E_HIP;
    }
    if (p->block.alloc(p->dev, 256) != hipSuccess) return SBLAS_E_HIP;
    p->flag = p->block.at<unsigned long long>();
    if (hipMemsetAsync(p->flag, 0xff, 256, s) != hipSuccess) return SBLAS_E_HIP;

    const int32_t *d_rowptr = rowptr, *d_colidx = colidx;
    const double *d_val = val; // theta > 0 on a smoothed plan: the level's values on the device, for the numeric chain
    int64_t nl = n, nnzl = nnz, nnz_most = nnz;
    DeviceBuffer val_here, val_next; // such a level's values, and the next one's
    // the device aggregation's scratch, sized by level 0 (the levels only shrink): agg | aggptr | members, and its workspace
    DeviceBuffer agg_tmp, agg_ws;
    const size_t agg_arr = ((size_t)n * 4 + 15) / 16 * 16, agg_ptr = (((size_t)n + 1) * 4 + 15) / 16 * 16;
    const size_t agg_ws_bytes = dev_agg ? sblas_hip_amg_aggregate_workspace(n, nnz) : 0;
    if (dev_agg && n > coarse_max && max_levels > 1 &&
        (agg_tmp.alloc(p->dev, 2 * agg_arr + agg_ptr) != hipSuccess || agg_ws.alloc(p->dev, agg_ws_bytes) != hipSuccess))
        return SBLAS_E_HIP;
    int32_t *const d_agg = agg_tmp ? agg_tmp.at<int32_t>() : nullptr, *const d_aggptr = agg_tmp ? agg_tmp.at<int32_t>(agg_arr) : nullptr;
    int32_t *const d_members = agg_tmp ? agg_tmp.at<int32_t>(agg_arr + agg_ptr) : nullptr;
    for (int l = 0;; ++l) {
        std::unique_ptr<AmgLevel> L(new AmgLevel);
        L->n = nl, L->nnz = nnzl, L->rowptr = d_rowptr, L->colidx = d_colidx;
        std::vector<int32_t> dpos((size_t)nl), agg, aggptr, members;
        int64_t bad = -1;
        if (!dev_agg || l == 0) {
            rc = sblas_ilu0_check(nl, h_rowptr.data(), h_colidx.data(), dpos.data(), &bad);
            if (rc != SBLAS_OK) { // level 0: the caller's structure; below it cannot happen (the COO plan sorts, a diagonal is always present)
                if (bad_row) *bad_row = bad;
                return rc;
            }
        }
        std::vector<int32_t> c_rowptr, c_colidx;
        std::vector<double> c_val;
        int64_t nnz_next = 0;
        // the triplets of this level's COO plan: written on the host and uploaded, or by a kernel from the device's agg
        DeviceBuffer trip;
        int32_t *d_trow = nullptr, *d_tcol = nullptr;
        const auto make_triplets = [&](bool coarse_rows) -> int {
            if (dev_agg) {
                const size_t tr = ((size_t)nnzl * 4 + 15) / 16 * 16;
                if (trip.alloc(p->dev, 2 * tr + 16) != hipSuccess) return SBLAS_E_HIP;
                d_trow = trip.at<int32_t>(), d_tcol = trip.at<int32_t>(tr);
                if (nnzl == 0) return SBLAS_OK;
                if (coarse_rows) amg_triplets_kernel<true><<<grid_of(nnzl), AMG_THREADS, 0, s>>>(nnzl, nl, L->rowptr, L->colidx, d_agg, d_trow, d_tcol);
                else amg_triplets_kernel<false><<<grid_of(nnzl), AMG_THREADS, 0, s>>>(nnzl, nl, L->rowptr, L->colidx, d_agg, d_trow, d_tcol);
                return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
            }
            std::vector<int32_t> trow((size_t)nnzl), tcol((size_t)nnzl);
            for (int64_t i = 0; i < nl; ++i)
                for (int64_t e = h_rowptr[i]; e < h_rowptr[i + 1]; ++e)
                    trow[(size_t)e] = coarse_rows ? agg[(size_t)i] : (int32_t)i, tcol[(size_t)e] = agg[(size_t)h_colidx[e]];
            size_t tb = 0;
            Segment tseg[2] = {Segment(trow), Segment(tcol)};
            if (upload_segments(trip, p->dev, s, tseg, 2, &tb) != hipSuccess) return SBLAS_E_HIP;
            d_trow = trip.at<int32_t>(), d_tcol = trip.at<int32_t>(tseg[1].offset);
            return SBLAS_OK;
        };
        if (nl > coarse_max && l + 1 < max_levels) {
            int64_t nc = 0;
            if (dev_agg) {
                int64_t rounds = 0;
                rc = sblas_hip_amg_aggregate_i32(p->dev, s, nl, nnzl, d_rowptr, d_colidx, by_value ? d_val : nullptr, theta, seed, (uint32_t)l, d_agg,
                                                 d_aggptr, d_members, agg_ws.at<char>(), agg_ws_bytes, &nc, &rounds);
                if (rc != SBLAS_OK) return rc;
            } else {
                agg.resize((size_t)nl), members.resize((size_t)nl);
                nc = amg_aggregate(nl, h_rowptr.data(), h_colidx.data(), by_value ? h_val.data() : nullptr, theta, seed, (uint32_t)l, agg.data(), aggptr,
                                   members.data());
            }
            if (smoothed && amg_keep_level(nl, nc, min_reduction)) {
                L->n_coarse = nc; // the transfer operators and the products: after this level's own arrays are on the device
            } else if (!smoothed && amg_keep_level(nl, nc, min_reduction)) { // a level that does not reduce n (enough) is discarded
                rc = make_triplets(true);
                if (rc != SBLAS_OK) return rc;
                rc = sblas_hip_coo_plan_create(p->dev, s, nc, nc, nnzl, d_trow, d_tcol, SBLAS_COO_SUM, &L->coo);
                if (rc != SBLAS_OK) return rc;
                int64_t ci[8];
                const int32_t *c_rp = nullptr, *c_ci = nullptr, *c_perm = nullptr, *c_run = nullptr;
                sblas_hip_coo_plan_info(L->coo, ci);
                sblas_hip_coo_plan_csr(L->coo, &c_rp, &c_ci, &c_perm, &c_run);
                const int64_t nnzc = nnz_next = ci[3];
                int64_t cbad = -1;
                rc = dev_agg ? fetch_rowptr(s, nc, nnzc, c_rp, c_rowptr) : fetch_structure(s, nc, nnzc, c_rp, c_ci, c_rowptr, c_colidx, &cbad);
                if (rc != SBLAS_OK) return SBLAS_E_HIP;
                if (by_value && dev_agg) { // the coarse values of the strength test: the plan's own assembly, the same left-to-right sums
                    if (val_next.alloc(p->dev, (size_t)nnzc * 8 + 256) != hipSuccess) return SBLAS_E_HIP;
                    rc = sblas_hip_coo_plan_assemble(L->coo, s, d_val, val_next.at<double>());
                    if (rc != SBLAS_OK) return rc;
                } else if (by_value) { // the coarse values of the strength test, in the assemble order
                    std::vector<int32_t> perm((size_t)nnzl), run((size_t)nnzc + 1);
                    if (hipMemcpyAsync(perm.data(), c_perm, (size_t)nnzl * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                        hipMemcpyAsync(run.data(), c_run, ((size_t)nnzc + 1) * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                        hipStreamSynchronize(s) != hipSuccess)
                        return SBLAS_E_HIP;
                    c_val.resize((size_t)nnzc);
                    for (int64_t e = 0; e < nnzc; ++e) {
                        double v = h_val[(size_t)perm[(size_t)run[(size_t)e]]];
                        for (int64_t k = (int64_t)run[(size_t)e] + 1; k < run[(size_t)e + 1]; ++k) v = v + h_val[(size_t)perm[(size_t)k]];
                        c_val[(size_t)e] = v;
                    }
                }
                L->n_coarse = nc;
                d_rowptr = c_rp, d_colidx = c_ci;
            }
        }
        const bool last = L->n_coarse == 0;
        if (last) agg.clear(), aggptr.clear(), members.clear();
        // the rows packed as one wide level of a solve
        std::vector<int32_t> zero_level((size_t)nl, 0);
        LevelOrder o;
        std::vector<SweepUnit> units;
        const auto unit_of = [&](int32_t i, int32_t q) { return SweepUnit{i, h_rowptr[(size_t)i], h_rowptr[(size_t)i + 1], q}; };
        level_pack(nl, h_rowptr.data(), zero_level.data(), 1, unit_of, NO_SWEEP_UNIT, o, units);
        L->units = (int64_t)units.size();
        Segment seg[5] = {Segment(units), Segment(dpos), Segment(agg), Segment(aggptr), Segment(members)};
        size_t ib = 0;
        if (dev_agg) { // the same layout; only the units (and level 0's dpos) are uploaded, the rest is copied or made on the device
            const size_t nc = (size_t)L->n_coarse;
            seg[2].bytes = seg[4].bytes = (size_t)nl * 4, seg[3].bytes = (nc + 1) * 4;
            for (int k = 0; k < (last ? 2 : 5); ++k) seg[k].offset = ib, ib += (seg[k].bytes + 15) / 16 * 16;
            hipError_t e = L->ibuf.alloc(p->dev, ib);
            if (e == hipSuccess) e = hipMemcpyAsync(L->ibuf.at<char>(), units.data(), seg[0].bytes, hipMemcpyHostToDevice, s);
            if (e == hipSuccess && l == 0) e = hipMemcpyAsync(L->ibuf.at<char>(seg[1].offset), dpos.data(), seg[1].bytes, hipMemcpyHostToDevice, s);
            if (e == hipSuccess && l > 0) {
                amg_dpos_kernel<<<grid_of(nl), AMG_THREADS, 0, s>>>(nl, L->rowptr, L->colidx, L->ibuf.at<int32_t>(seg[1].offset));
                e = hipGetLastError();
            }
            if (e == hipSuccess && !last) e = hipMemcpyAsync(L->ibuf.at<char>(seg[2].offset), d_agg, seg[2].bytes, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess && !last) e = hipMemcpyAsync(L->ibuf.at<char>(seg[3].offset), d_aggptr, seg[3].bytes, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess && !last) e = hipMemcpyAsync(L->ibuf.at<char>(seg[4].offset), d_members, seg[4].bytes, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s); // the host vector of the units is read until here
            if (e != hipSuccess) return SBLAS_E_HIP;
        } else if (upload_segments(L->ibuf, p->dev, s, seg, last ? 2 : 5, &ib) != hipSuccess) return SBLAS_E_HIP; // the coarsest has no aggregates
        L->d_units = L->ibuf.at<SweepUnit>(), L->dpos = L->ibuf.at<int32_t>(seg[1].offset);
        if (!last) L->agg = L->ibuf.at<int32_t>(seg[2].offset), L->aggptr = L->ibuf.at<int32_t>(seg[3].offset), L->members = L->ibuf.at<int32_t>(seg[4].offset);
        // doubles: wd | x0 | x1 (below level 0) | res (above the coarsest) | b, val (below level 0)
        const size_t vec = ((size_t)nl * 8 + 255) / 256 * 256, vals = ((size_t)nnzl * 8 + 255) / 256 * 256;
        const size_t db = vec * (2 + (l > 0 ? 2 : 0) + (last ? 0 : 1)) + (l > 0 ? vals : 0);
        if (L->dbuf.alloc(p->dev, db) != hipSuccess) return SBLAS_E_HIP;
        size_t off = 0;
        const auto take = [&](size_t bytes) {
            double *q = L->dbuf.at<double>(off);
            off += bytes;
            return q;
        };
        L->wd = take(vec), L->x[0] = take(vec);
        if (l > 0) L->x[1] = take(vec), L->b = take(vec);
        if (!last) L->res = take(vec);
        if (l > 0) L->own_val = take(vals), L->val = L->own_val;
        L->bytes = ib + db;
        if (smoothed && !last) {
            const int64_t nc = L->n_coarse;
            // P_l: the COO plan of (row(e), agg[col(e)]) in stored order
            rc = make_triplets(false);
            if (rc != SBLAS_OK) return rc;
            rc = sblas_hip_coo_plan_create(p->dev, s, nl, nc, nnzl, d_trow, d_tcol, SBLAS_COO_SUM, &L->coo);
            if (rc != SBLAS_OK) return rc;
            int64_t ci[8], gi[12];
            sblas_hip_coo_plan_info(L->coo, ci);
            sblas_hip_coo_plan_csr(L->coo, &L->p_rowptr, &L->p_colidx, nullptr, nullptr);
            const int64_t nnzp = L->nnz_p = ci[3];
            L->bytes += (size_t)ci[6];
            // the units of P's rows, and of R's once its row pointer is known; R_l = P_l^T by the device transpose
            std::vector<int32_t> hp_rowptr, hp_colidx, hr_rowptr((size_t)nc + 1);
            int64_t pbad = -1;
            if ((dev_agg ? fetch_rowptr(s, nl, nnzp, L->p_rowptr, hp_rowptr) : fetch_structure(s, nl, nnzp, L->p_rowptr, L->p_colidx, hp_rowptr, hp_colidx, &pbad)) != SBLAS_OK)
                return SBLAS_E_HIP;
            const size_t i_rp = ((size_t)nc + 1 + 3) / 4 * 4, i_e = ((size_t)nnzp + 3) / 4 * 4; // int32 counts, 16-byte steps
            DeviceBuffer tws;
            const size_t ws_bytes = sblas_hip_csr_transpose_workspace(nl, nc, nnzp);
            if (tws.alloc(p->dev, ws_bytes ? ws_bytes : 16) != hipSuccess) return SBLAS_E_HIP;
            const size_t rbytes = (i_rp + 2 * i_e) * 4 + 16; // r_rowptr | r_colidx | r_perm
            if (L->tbuf.alloc(p->dev, rbytes) != hipSuccess) return SBLAS_E_HIP;
            L->r_rowptr = L->tbuf.at<int32_t>(), L->r_colidx = L->tbuf.at<int32_t>(i_rp * 4), L->r_perm = L->tbuf.at<int32_t>((i_rp + i_e) * 4);
            rc = sblas_hip_csr_transpose_f64_i32(p->dev, s, nl, nc, nnzp, L->p_rowptr, L->p_colidx, nullptr, L->r_rowptr, L->r_colidx, nullptr,
                                                 L->r_perm, tws.at<char>(), ws_bytes);
            if (rc != SBLAS_OK) return rc;
            if (hipMemcpyAsync(hr_rowptr.data(), L->r_rowptr, ((size_t)nc + 1) * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipStreamSynchronize(s) != hipSuccess)
                return SBLAS_E_HIP;
            std::vector<int32_t> zero_p((size_t)nl, 0), zero_r((size_t)nc, 0);
            LevelOrder op, orr;
            std::vector<SweepUnit> p_units, r_units;
            const auto p_unit = [&](int32_t i, int32_t q) { return SweepUnit{i, hp_rowptr[(size_t)i], hp_rowptr[(size_t)i + 1], q}; };
            const auto r_unit = [&](int32_t i, int32_t q) { return SweepUnit{i, hr_rowptr[(size_t)i], hr_rowptr[(size_t)i + 1], q}; };
            level_pack(nl, hp_rowptr.data(), zero_p.data(), 1, p_unit, NO_SWEEP_UNIT, op, p_units);
            level_pack(nc, hr_rowptr.data(), zero_r.data(), 1, r_unit, NO_SWEEP_UNIT, orr, r_units);
            L->p_units = (int64_t)p_units.size(), L->r_units = (int64_t)r_units.size();
            Segment useg[2] = {Segment(p_units), Segment(r_units)};
            size_t ub = 0;
            if (upload_segments(L->ubuf, p->dev, s, useg, 2, &ub) != hipSuccess) return SBLAS_E_HIP;
            L->d_p_units = L->ubuf.at<SweepUnit>(), L->d_r_units = L->ubuf.at<SweepUnit>(useg[1].offset);
            // the products' plans: A_l P_l, then R_l (A_l P_l); a product too large for int32 is refused there
            rc = sblas_hip_spgemm_plan_create(p->dev, s, nl, nl, nc, d_rowptr, d_colidx, L->p_rowptr, L->p_colidx, SBLAS_SPGEMM_AUTO, 0, &L->ap);
            if (rc != SBLAS_OK) return rc;
            const int32_t *ap_rp = nullptr, *ap_ci = nullptr, *c_rp = nullptr, *c_ci = nullptr;
            sblas_hip_spgemm_plan_info(L->ap, gi);
            sblas_hip_spgemm_plan_csr(L->ap, &ap_rp, &ap_ci);
            L->nnz_ap = gi[3], L->bytes += (size_t)gi[10];
            rc = sblas_hip_spgemm_plan_create(p->dev, s, nc, nl, nc, L->r_rowptr, L->r_colidx, ap_rp, ap_ci, SBLAS_SPGEMM_AUTO, 0, &L->rap);
            if (rc != SBLAS_OK) return rc;
            sblas_hip_spgemm_plan_info(L->rap, gi);
            sblas_hip_spgemm_plan_csr(L->rap, &c_rp, &c_ci);
            const int64_t nnzc = nnz_next = gi[3];
            L->bytes += (size_t)gi[10];
            int64_t cbad = -1;
            if ((dev_agg ? fetch_rowptr(s, nc, nnzc, c_rp, c_rowptr) : fetch_structure(s, nc, nnzc, c_rp, c_ci, c_rowptr, c_colidx, &cbad)) != SBLAS_OK)
                return SBLAS_E_HIP;
            const size_t v_p = ((size_t)nnzp * 8 + 255) / 256 * 256, v_ap = ((size_t)L->nnz_ap * 8 + 255) / 256 * 256;
            if (L->tval.alloc(p->dev, 2 * v_p + v_ap + 256) != hipSuccess) return SBLAS_E_HIP;
            L->p_val = L->tval.at<double>(), L->r_val = L->tval.at<double>(v_p), L->ap_val = L->tval.at<double>(2 * v_p);
            L->bytes += rbytes + ub + 2 * v_p + v_ap + 256;
            if (by_value) { // the coarse values of the next level's strength test: the numeric chain, once, on the given values
                DeviceBuffer t_tmp;
                if (t_tmp.alloc(p->dev, (size_t)nnzl * 8 + 256) != hipSuccess || val_next.alloc(p->dev, (size_t)nnzc * 8 + 256) != hipSuccess)
                    return SBLAS_E_HIP;
                launch_pvalues(s, *L, p->omega_p, d_val, t_tmp.at<double>());
                rc = smoothed_values(s, *p, *L, d_val, t_tmp.at<double>(), val_next.at<double>());
                if (rc != SBLAS_OK) return rc;
                if (!dev_agg) c_val.resize((size_t)nnzc); // the host rule reads them; the device's aggregation reads val_next in place
                if ((!dev_agg && hipMemcpyAsync(c_val.data(), val_next.at<double>(), (size_t)nnzc * 8, hipMemcpyDeviceToHost, s) != hipSuccess) ||
                    hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess)
                    return SBLAS_E_HIP;
            }
            d_rowptr = c_rp, d_colidx = c_ci;
            if (nnzc > nnz_most) nnz_most = nnzc;
        }
        p->lv.push_back(std::move(L));
        if (last) break;
        nl = p->lv.back()->n_coarse, nnzl = nnz_next;
        h_rowptr.swap(c_rowptr), h_colidx.swap(c_colidx), h_val.swap(c_val);
        if (by_value && (smoothed || dev_agg)) { // the next level's values stay on the device for its own chain (and aggregation)
            DeviceBuffer done(std::move(val_here));
            val_here = std::move(val_next);
            d_val = val_here.at<double>();
        }
    }
    if (smoothed) {
        p->t_bytes = (size_t)nnz_most * 8 + 256;
        if (p->tscratch.alloc(p->dev, p->t_bytes) != hipSuccess) return SBLAS_E_HIP;
        p->t = p->tscratch.at<double>();
    }
    if (hipStreamSynchronize(s) != hipSuccess) return SBLAS_E_HIP;
    *plan_out = p.release();
    return SBLAS_OK;
}

int sblas_hip_amg_plan_info(const void *plan, int64_t out[12])
{
    if (!plan || !out) return SBLAS_E_INVALID;
    const AmgPlan *p = static_cast<const AmgPlan *>(plan);
    int64_t rows = 0, entries = 0, bytes = (p->flag ? 256 : 0) + (int64_t)p->t_bytes + (int64_t)p->cheb_bytes;
    for (const auto &L : p->lv) rows += L->n, entries += L->nnz, bytes += (int64_t)L->bytes + (int64_t)L->cheb_bytes;
    out[0] = p->n, out[1] = p->nnz, out[2] = p->levels(), out[3] = p->nu, out[4] = p->coarse_sweeps;
    out[5] = p->degree ? sblas_amg_launches_cheb(p->levels(), p->nu, p->coarse_sweeps, p->degree) : sblas_amg_launches(p->levels(), p->nu, p->coarse_sweeps);
    out[6] = rows, out[7] = entries, out[8] = bytes, out[9] = p->smoother, out[10] = p->ready, out[11] = p->lv.empty() ? 0 : p->lv.back()->n;
    return SBLAS_OK;
}

int sblas_hip_amg_plan_level(const void *plan, int level, int64_t sizes[4], const void *ptrs[7])
{
    const AmgPlan *p = static_cast<const AmgPlan *>(plan);
    if (!p || !sizes || !ptrs || level < 0 || level >= p->levels()) return SBLAS_E_INVALID;
    const AmgLevel &L = *p->lv[(size_t)level];
    sizes[0] = L.n, sizes[1] = L.nnz, sizes[2] = L.n_coarse, sizes[3] = L.units;
    ptrs[0] = L.rowptr, ptrs[1] = L.colidx, ptrs[2] = L.val, ptrs[3] = L.wd, ptrs[4] = L.agg, ptrs[5] = L.aggptr, ptrs[6] = L.members;
    return SBLAS_OK;
}

int sblas_hip_amg_plan_transfer(const void *plan, int level, int64_t sizes[3], const void *ptrs[6])
{
    const AmgPlan *p = static_cast<const AmgPlan *>(plan);
    if (!p || !sizes || !ptrs || !p->smoothed() || level < 0 || level + 1 >= p->levels()) return SBLAS_E_INVALID;
    const AmgLevel &L = *p->lv[(size_t)level];
    sizes[0] = L.n, sizes[1] = L.n_coarse, sizes[2] = L.nnz_p;
    ptrs[0] = L.p_rowptr, ptrs[1] = L.p_colidx, ptrs[2] = L.p_val, ptrs[3] = L.r_rowptr, ptrs[4] = L.r_colidx, ptrs[5] = L.r_val;
    return SBLAS_OK;
}

int sblas_hip_amg_plan_options(const void *plan, double out[4])
{
    const AmgPlan *p = static_cast<const AmgPlan *>(plan);
    if (!p || !out) return SBLAS_E_INVALID;
    out[0] = (double)p->prolongator, out[1] = p->omega_p, out[2] = p->min_reduction, out[3] = (double)p->aggregation;
    return SBLAS_OK;
}

int sblas_hip_amg_plan_speaks_for(const void *plan, int dev, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx)
{
    const AmgPlan *p = static_cast<const AmgPlan *>(plan);
    if (!p || p->dev != resolve_device(dev)) return SBLAS_E_INVALID;
    return n == p->n && nnz == p->nnz && rowptr == p->rowptr && colidx == p->colidx ? SBLAS_OK : SBLAS_E_INVALID;
}

int sblas_hip_amg_plan_destroy(void *plan)
{
    delete static_cast<AmgPlan *>(plan);
    return SBLAS_OK;
}

int sblas_hip_amg_plan_setup(void *plan, void *stream, const double *val, int smoother, double omega, int nu, int coarse_sweeps,
                             double coarse_scale)
{
    if (smoother != SBLAS_AMG_JACOBI && smoother != SBLAS_AMG_L1) return SBLAS_E_INVALID;
    return sblas_hip_amg_plan_setup_ex(plan, stream, val, smoother, omega, nu, coarse_sweeps, coarse_scale, 0, 0, 0.0, 0.0);
}

namespace {

// The Chebyshev smoother's buffers, once a plan: a level's direction vector, scalar block and partial sums, and the
// estimate's four work vectors sized by level 0.  An allocation: refused while the stream is capturing.
int cheb_allocate(AmgPlan *p, hipStream_t s)
{
    if (p->ebuf) return SBLAS_OK;
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &capturing) != hipSuccess) return SBLAS_E_HIP;
    if (capturing != hipStreamCaptureStatusNone) return SBLAS_E_INVALID;
    const auto pad = [](size_t b) { return (b + 255) / 256 * 256; };
    for (auto &Lp : p->lv) {
        AmgLevel &L = *Lp;
        const size_t vec = pad((size_t)L.n * 8), block = pad((size_t)CHEBY_BLOCK_SLOTS * 8), part = pad((size_t)krylov_cells(L.n) * 8);
        if (!L.cbuf && L.cbuf.alloc(p->dev, vec + block + part) != hipSuccess) return SBLAS_E_HIP; // kept if a later one fails
        L.d = L.cbuf.at<double>();
        L.cheb.n = L.n, L.cheb.units = L.units, L.cheb.d_units = L.d_units, L.cheb.rowptr = L.rowptr, L.cheb.colidx = L.colidx, L.cheb.dpos = L.dpos;
        L.cheb.dinv = L.wd, L.cheb.blk = L.cbuf.at<double>(vec), L.cheb.part = L.cbuf.at<double>(vec + block);
        L.cheb_bytes = vec + block + part;
        if (hipMemsetAsync(L.cheb.blk, 0, block, s) != hipSuccess) return SBLAS_E_HIP;
    }
    const size_t vec0 = pad((size_t)p->n * 8);
    if (p->ebuf.alloc(p->dev, 4 * vec0) != hipSuccess) return SBLAS_E_HIP;
    for (int k = 0; k < 4; ++k) p->est[k] = p->ebuf.at<double>((size_t)k * vec0);
    p->cheb_bytes = 4 * vec0;
    return SBLAS_OK;
}

} // namespace

int sblas_hip_amg_plan_setup_ex(void *plan, void *stream, const double *val, int smoother, double omega, int nu, int coarse_sweeps,
                                double coarse_scale, int degree, int eig_steps, double eig_boost, double eig_ratio)
{
    AmgPlan *p = static_cast<AmgPlan *>(plan);
    if (!p) return SBLAS_E_INVALID;
    const bool cheb = smoother == SBLAS_AMG_CHEBYSHEV;
    if (smoother != SBLAS_AMG_JACOBI && smoother != SBLAS_AMG_L1 && !cheb) return SBLAS_E_INVALID;
    if (!(omega >= 0.0) || !isfinite(omega) || !isfinite(coarse_scale)) return SBLAS_E_INVALID;
    if (!amg_cycle_args_ok(p->levels(), nu, coarse_sweeps)) return SBLAS_E_INVALID;
    if (cheb && (omega != 0.0 || !amg_cheb_args_ok(degree, coarse_sweeps) || !cheby_steps_ok(eig_steps) || !cheby_boost_ok(eig_boost) ||
                 !cheby_ratio_ok(eig_ratio)))
        return SBLAS_E_INVALID; // omega is left unset with the polynomial
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    if (p->n > 0 && !val) return SBLAS_E_INVALID;
    if (omega == 0.0) omega = smoother == SBLAS_AMG_L1 ? 1.0 : 2.0 / 3.0;
    hipStream_t s = (hipStream_t)stream;
    if (cheb && p->n > 0) {
        const int rc = cheb_allocate(p, s);
        if (rc != SBLAS_OK) return rc;
    }
    p->ready = false;
    p->smoother = smoother, p->omega = cheb ? 0.0 : omega, p->nu = nu, p->coarse_sweeps = coarse_sweeps, p->scale = coarse_scale;
    p->degree = cheb ? degree : 0;
    if (p->n == 0) {
        p->ready = true;
        return SBLAS_OK;
    }
    if (hipMemsetAsync(p->flag, 0xff, 8, s) != hipSuccess) return SBLAS_E_HIP;
    p->lv[0]->val = val;
    for (int l = 0; l < p->levels(); ++l) {
        AmgLevel &L = *p->lv[(size_t)l];
        if (cheb) { // wd = 1 / a_ii, the level's estimate (salt seed + l) and its table; the coarsest's has coarse_sweeps entries
            L.cheb.val = L.val;
            cheby_setup_launches(s, L.cheb, p->flag, l, p->seed, eig_steps, eig_boost, eig_ratio, (double)NAN, l + 1 == p->levels() ? coarse_sweeps : degree,
                                 p->est[0], p->est[1], p->est[2], p->est[3]);
        } else {
            amg_wd_kernel<<<grid_of(L.n), AMG_THREADS, 0, s>>>(L.n, l, smoother, omega, L.rowptr, L.dpos, L.val, L.wd, p->flag);
        }
        if (l + 1 < p->levels()) {
            double *coarse = p->lv[(size_t)l + 1]->own_val;
            if (p->smoothed()) launch_pvalues(s, L, p->omega_p, L.val, p->t);
            const int rc = p->smoothed() ? smoothed_values(s, *p, L, L.val, p->t, coarse) : sblas_hip_coo_plan_assemble(L.coo, s, L.val, coarse);
            if (rc != SBLAS_OK) return rc;
        }
    }
    if (hipGetLastError() != hipSuccess) return SBLAS_E_HIP;
    p->ready = true;
    return SBLAS_OK;
}

int sblas_hip_amg_plan_apply(const void *plan, void *stream, const double *r, double *z)
{
    const AmgPlan *p = static_cast<const AmgPlan *>(plan);
    if (!p || !p->ready) return SBLAS_E_INVALID;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    if (p->n == 0) return SBLAS_OK;
    if (!r || !z || overlap(r, z, p->n)) return SBLAS_E_INVALID;
    DeviceOps ops{p, (hipStream_t)stream, r, z};
    amg_cycle(p->levels(), p->nu, p->coarse_sweeps, ops, 0, p->degree);
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_amg_plan_check(const void *plan, void *stream, int64_t out[2])
{
    const AmgPlan *p = static_cast<const AmgPlan *>(plan);
    if (!p || !out) return SBLAS_E_INVALID;
    out[0] = out[1] = -1;
    if (p->n == 0) return SBLAS_OK;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    unsigned long long w = FLAG_CLEAN;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(&w, p->flag, 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return SBLAS_E_HIP;
    if (w != FLAG_CLEAN) out[0] = (int64_t)(w >> 32), out[1] = (int64_t)(w & 0xffffffffull);
    return SBLAS_OK;
}

int sblas_hip_amg_plan_eig(const void *plan, void *stream, int level, double out[4], double *table, int *entries)
{
    const AmgPlan *p = static_cast<const AmgPlan *>(plan);
    if (!p || !out || !p->ready || p->degree == 0 || level < 0 || level >= p->levels()) return SBLAS_E_INVALID;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    const AmgLevel &L = *p->lv[(size_t)level];
    const int count = level + 1 == p->levels() ? p->coarse_sweeps : p->degree;
    double h[CS_ALPHAS];
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(h, L.cheb.blk, sizeof h, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && table) e = hipMemcpyAsync(table, L.cheb.blk + CS_TABLE, (size_t)count * 16, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return SBLAS_E_HIP;
    long long m;
    memcpy(&m, &h[CS_M], 8);
    out[0] = (double)m, out[1] = h[CS_RITZ], out[2] = h[CS_G], out[3] = h[CS_LMAX];
    if (entries) *entries = count;
    return SBLAS_OK;
}

int sblas_hip_amg_sweep_f64(const void *plan, void *stream, int level, int mode, const double *b, const double *x, double *y)
{
    const AmgLevel *L = level_of(plan, level, true);
    if (!L || mode < MODE_SWEEP || mode > MODE_FIRST) return SBLAS_E_INVALID;
    if (L->n == 0) return SBLAS_OK;
    if (!b || !y || overlap(b, y, L->n) || (mode != MODE_FIRST && (!x || overlap(x, y, L->n)))) return SBLAS_E_INVALID;
    launch_sweep((hipStream_t)stream, *L, mode, b, x, y);
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_amg_restrict_f64(const void *plan, void *stream, int level, const double *res, double *bc)
{
    const AmgLevel *L = level_of(plan, level, false);
    if (!L || L->n_coarse == 0 || !res || !bc) return SBLAS_E_INVALID;
    if (static_cast<const AmgPlan *>(plan)->smoothed() && (!static_cast<const AmgPlan *>(plan)->ready || res == bc)) return SBLAS_E_INVALID; // R's values are setup's
    launch_restrict((hipStream_t)stream, *static_cast<const AmgPlan *>(plan), *L, res, bc);
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_amg_prolong_f64(const void *plan, void *stream, int level, double scale, const double *e, double *x)
{
    const AmgLevel *L = level_of(plan, level, false);
    if (!L || L->n_coarse == 0 || !e || !x) return SBLAS_E_INVALID;
    if (static_cast<const AmgPlan *>(plan)->smoothed() && (!static_cast<const AmgPlan *>(plan)->ready || e == x)) return SBLAS_E_INVALID; // P's values are setup's
    launch_prolong((hipStream_t)stream, *static_cast<const AmgPlan *>(plan), *L, scale, e, x);
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_amg_pvalues_f64(const void *plan, void *stream, int level, const double *val, double *t)
{
    const AmgLevel *L = level_of(plan, level, false);
    if (!L || !static_cast<const AmgPlan *>(plan)->smoothed()) return SBLAS_E_INVALID;
    if (L->nnz == 0) return SBLAS_OK;
    if (!val || !t || overlap(val, t, L->nnz)) return SBLAS_E_INVALID;
    launch_pvalues((hipStream_t)stream, *L, static_cast<const AmgPlan *>(plan)->omega_p, val, t);
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

} // extern "C"

// ---- the block cycle (include/sblas_hip_amg_multi.h) ---------------------------------------------------
extern "C" {

int sblas_hip_amg_plan_reserve_multi(void *plan, void *stream, int nrhs)
{
    AmgPlan *p = static_cast<AmgPlan *>(plan);
    if (!p || !amg_multi_width_ok(nrhs)) return SBLAS_E_INVALID;
    if (nrhs <= p->multi_width) return SBLAS_OK; // only grows
    if (p->n > 0) {
        if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
        hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing((hipStream_t)stream, &capturing) != hipSuccess) return SBLAS_E_HIP;
        if (capturing != hipStreamCaptureStatusNone) return SBLAS_E_INVALID; // an allocation
        // every level's new buffer first: the plan keeps what it had if one of them fails
        std::vector<DeviceBuffer> fresh(p->lv.size());
        std::vector<size_t> vec(p->lv.size());
        size_t bytes = 0;
        for (size_t l = 0; l < p->lv.size(); ++l) {
            vec[l] = ((size_t)p->lv[l]->n * (size_t)nrhs * 8 + 255) / 256 * 256;
            if (fresh[l].alloc(p->dev, 4 * vec[l]) != hipSuccess) return SBLAS_E_HIP;
            bytes += 4 * vec[l];
        }
        for (size_t l = 0; l < p->lv.size(); ++l) {
            AmgLevel &L = *p->lv[l];
            L.mbuf = std::move(fresh[l]);
            L.mx[0] = L.mbuf.at<double>(), L.mx[1] = L.mbuf.at<double>(vec[l]), L.mres = L.mbuf.at<double>(2 * vec[l]), L.mb = L.mbuf.at<double>(3 * vec[l]);
        }
        p->multi_bytes = bytes;
    }
    p->multi_width = nrhs;
    return SBLAS_OK;
}

int sblas_hip_amg_plan_multi_info(const void *plan, int64_t out[4])
{
    const AmgPlan *p = static_cast<const AmgPlan *>(plan);
    if (!p || !out) return SBLAS_E_INVALID;
    int64_t info[12];
    sblas_hip_amg_plan_info(plan, info);
    out[0] = p->multi_width, out[1] = (int64_t)p->multi_bytes, out[2] = info[5], out[3] = 0;
    return SBLAS_OK;
}

int sblas_hip_amg_plan_apply_multi(const void *plan, void *stream, int nrhs, const double *R, int64_t ldr, double *Z, int64_t ldz)
{
    const AmgPlan *p = static_cast<const AmgPlan *>(plan);
    if (!p || !p->ready || !amg_multi_width_ok(nrhs)) return SBLAS_E_INVALID;
    if (p->degree > 0) return SBLAS_E_INVALID; // the Chebyshev smoother has no block form
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    if (ldr < nrhs || ldz < nrhs) return SBLAS_E_INVALID;
    if (nrhs > p->multi_width) return SBLAS_E_WORKSPACE;
    if (p->n == 0) return SBLAS_OK;
    if (!block_ok(R, ldr, nrhs) || !block_ok(Z, ldz, nrhs) || blocks_overlap(R, p->n, ldr, Z, p->n, ldz, nrhs)) return SBLAS_E_INVALID;
    for (const auto &L : p->lv)
        if (!multi_grids_ok(*L, nrhs)) return SBLAS_E_INVALID;
    MultiOps ops{p, (hipStream_t)stream, nrhs, Blk{R, ldr}, Z, ldz};
    amg_cycle(p->levels(), p->nu, p->coarse_sweeps, ops, 0, 0);
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_amg_sweep_multi_f64(const void *plan, void *stream, int level, int mode, int nrhs, const double *B, int64_t ldb, const double *X,
                                  int64_t ldx, double *Y, int64_t ldy)
{
    const AmgLevel *L = level_of(plan, level, true);
    if (!L || mode < MODE_SWEEP || mode > MODE_FIRST || !amg_multi_width_ok(nrhs)) return SBLAS_E_INVALID;
    const bool first = mode == MODE_FIRST;
    if (ldb < nrhs || ldy < nrhs || (!first && ldx < nrhs)) return SBLAS_E_INVALID;
    if (L->n == 0) return SBLAS_OK;
    if (!block_ok(B, ldb, nrhs) || !block_ok(Y, ldy, nrhs) || blocks_overlap(B, L->n, ldb, Y, L->n, ldy, nrhs)) return SBLAS_E_INVALID;
    if (!first && (!block_ok(X, ldx, nrhs) || blocks_overlap(X, L->n, ldx, Y, L->n, ldy, nrhs))) return SBLAS_E_INVALID;
    if (!multi_grids_ok(*L, nrhs)) return SBLAS_E_INVALID;
    launch_sweep_multi((hipStream_t)stream, *L, mode, nrhs, Blk{B, ldb}, Blk{first ? nullptr : X, first ? 0 : ldx}, Y, ldy);
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_amg_restrict_multi_f64(const void *plan, void *stream, int level, int nrhs, const double *RES, int64_t ldr, double *BC, int64_t ldc)
{
    const AmgLevel *L = level_of(plan, level, false);
    const AmgPlan *p = static_cast<const AmgPlan *>(plan);
    if (!L || L->n_coarse == 0 || !amg_multi_width_ok(nrhs) || !block_ok(RES, ldr, nrhs) || !block_ok(BC, ldc, nrhs)) return SBLAS_E_INVALID;
    if (p->smoothed() && !p->ready) return SBLAS_E_INVALID; // R's values are setup's
    if (blocks_overlap(RES, L->n, ldr, BC, L->n_coarse, ldc, nrhs) || !multi_grids_ok(*L, nrhs)) return SBLAS_E_INVALID;
    launch_restrict_multi((hipStream_t)stream, *p, *L, nrhs, Blk{RES, ldr}, BC, ldc);
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_amg_prolong_multi_f64(const void *plan, void *stream, int level, double scale, int nrhs, const double *E, int64_t lde, double *X,
                                    int64_t ldx)
{
    const AmgLevel *L = level_of(plan, level, false);
    const AmgPlan *p = static_cast<const AmgPlan *>(plan);
    if (!L || L->n_coarse == 0 || !amg_multi_width_ok(nrhs) || !block_ok(E, lde, nrhs) || !block_ok(X, ldx, nrhs)) return SBLAS_E_INVALID;
    if (p->smoothed() && !p->ready) return SBLAS_E_INVALID; // P's values are setup's
    if (blocks_overlap(E, L->n_coarse, lde, X, L->n, ldx, nrhs) || !multi_grids_ok(*L, nrhs)) return SBLAS_E_INVALID;
    launch_prolong_multi((hipStream_t)stream, *p, *L, nrhs, scale, Blk{E, lde}, X, ldx);
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

} // extern "C"
