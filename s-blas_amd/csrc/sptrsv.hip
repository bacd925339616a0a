// sptrsv.hip -- sparse triangular solves on a level-scheduled plan: T x = alpha b (SpSV) and
// T X = alpha B for nrhs right-hand sides (SpSM), T the lower or upper triangle of a square CSR matrix.
//
// The plan sorts the rows by (level, row) once (the host rule: sptrsv_plan.cpp); a solve is then a fixed sequence of
// launches of two kernels:
//   wide   one level a launch; the level's rows, in ascending row order, spread over the grid;
//   chain  one workgroup walks a run of consecutive levels with __syncthreads() between them.
// Nothing waits across workgroups: no flag polling, no cooperative launch, no grid barrier, no atomics.  The only
// synchronisation is the kernel boundary and __syncthreads(), and every loop's trip count comes from the plan.
//
// Visibility inside a chain launch: x is written with plain global stores and read with plain global loads.
// __syncthreads() is a workgroup-scope release and acquire around the barrier: every wave waits for its stores
// (s_waitcnt vmcnt(0)) before it arrives, and no load of x for a later level is issued before it leaves (what is fetched
// ahead of the barrier is plan data, which no kernel writes).  The waves of one
// workgroup run on one CU and share its vector L1, which is write-through and sees the CU's own stores; the hazard of a
// stale L1 line exists only between CUs, and no other workgroup runs in a chain launch.  Between launches the kernel
// boundary orders everything.  x and b are not __restrict__: they may be the same array, and x is read and written in
// one launch.
//
// Results contract: solve_row() is the one expression of x[i], shared by both kernels.  Its bits are a function of the
// row's stored entries (columns and values, in stored order), the x values they name, b[i] and alpha: the lane group's
// width G(p) depends on the stored length p alone, lane l takes the entries l, l + G, ... in stored order with one fused
// multiply-add each, and the lanes fold by the butterfly of rowwise.h.  A level packs its rows, each with its own G(p)
// lanes, side by side: which rows share a wave does not enter any row's sum.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <memory>
#include <vector>
#include "../../include/sblas_hip.h"
#include "capi_util.h"
#include "rowwise.h"
#include "sptrsv.h"

using namespace sblas;

namespace {

constexpr int WIDE_THREADS = 256;

// a row as the SpSM kernels meet it, in (level, row) order: one 16-byte load
struct RowDesc {
    int32_t row, beg, end, diag; // diag: position of the stored diagonal in val, -1 under SBLAS_DIAG_UNIT
};
static_assert(sizeof(RowDesc) == 16, "one 16-byte load per row");

__device__ __forceinline__ RowDesc load_desc(const RowDesc *__restrict__ desc, int64_t k)
{
    const int4 v = *reinterpret_cast<const int4 *>(desc + k);
    return RowDesc{v.x, v.y, v.z, v.w};
}

__device__ __forceinline__ double finish_row(double alpha, double bi, double sum, double pivot)
{
#pragma clang fp contract(off) // three roundings, on every path: alpha * b, the subtraction, the division
    const double t = alpha * bi;
    return (t - sum) / pivot;
}

// A unit is four lanes of a launch.  A row of G(p) lanes is G(p) / 4 consecutive units, aligned to G(p) lanes inside its
// level; a unit that pads that alignment has row = -1.  tag: in a row's first unit the position of the stored diagonal in
// val (-1 under SBLAS_DIAG_UNIT); in its unit number s > 0, -2 - s.
struct Unit {
    int32_t row, beg, end, tag;
};
static_assert(sizeof(Unit) == 16, "one 16-byte load per unit");
constexpr Unit NO_UNIT{-1, 0, 0, -1};

__device__ __forceinline__ Unit load_unit(const Unit *__restrict__ units, int64_t u)
{
    const int4 v = *reinterpret_cast<const int4 *>(units + u);
    return Unit{v.x, v.y, v.z, v.w};
}

// x[row] for the row of unit u.  Every lane of the wave calls this together (the butterfly moves data between lanes);
// `quad` is the lane's place in its unit.
__device__ __forceinline__ void solve_row(const Unit u, int quad, bool lower, const int32_t *__restrict__ colidx,
                                          const double *__restrict__ val, double alpha, const double *b, double *x)
{
    const int gs = sptrsv_group_shift((int64_t)u.end - u.beg), G = 1 << gs;
    const int lane = (u.tag <= -2 ? 4 * (-2 - u.tag) : 0) + quad; // the lane's place among the row's G lanes
    const bool writer = u.row >= 0 && lane == 0;
    // the row's pivot and right-hand side travel with its first entries instead of waiting behind the fold
    const double pivot = writer && u.tag >= 0 ? val[u.tag] : 1.0;
    const double bi = writer ? b[u.row] : 0.0; // read before x[row] is written: in place is fine
    double s = 0.0;
    if (u.row >= 0) {
        for (int64_t e = (int64_t)u.beg + lane; e < u.end; e += G) {
            const int c = colidx[e];
            if (lower ? c < u.row : c > u.row) s = __builtin_fma(val[e], x[c], s); // the other triangle is never loaded
        }
    }
    const double f4 = fold_sum<4>(s);
    double f16 = f4 + lane_partner<4>(f4);
    f16 += lane_partner<8>(f16);
    double f64 = f16 + lane_partner<16>(f16);
    f64 += lane_partner<32>(f64);
    if (writer) x[u.row] = finish_row(alpha, bi, gs == 2 ? f4 : gs == 4 ? f16 : f64, pivot);
}

// Row `row` of X for one row: a lane per right-hand side, the stored entries one after another.  Column j's bits depend
// on column j of B alone.
__device__ __forceinline__ void solve_row_m(const RowDesc d, int lane, int lanes, bool lower, const int32_t *__restrict__ colidx,
                                            const double *__restrict__ val, int64_t nrhs, double alpha, const double *B, int64_t ldb,
                                            double *X, int64_t ldx)
{
    const double pivot = d.diag >= 0 ? val[d.diag] : 1.0;
    for (int64_t j = lane; j < nrhs; j += lanes) {
        double s = 0.0;
        int64_t e = d.beg;
        // four entries a round: their columns and values first, then the X values they select, so that four loads are in
        // flight where one was; the sum takes them one after another all the same
        for (; e + 4 <= d.end; e += 4) {
            int c[4];
            double v[4], xv[4];
            bool take[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) c[q] = colidx[e + q], v[q] = val[e + q];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                take[q] = lower ? c[q] < d.row : c[q] > d.row;
                xv[q] = take[q] ? X[(int64_t)c[q] * ldx + j] : 0.0; // the other triangle is never loaded
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) s = take[q] ? __builtin_fma(v[q], xv[q], s) : s;
        }
        for (; e < d.end; ++e) {
            const int c = colidx[e];
            if (lower ? c < d.row : c > d.row) s = __builtin_fma(val[e], X[(int64_t)c * ldx + j], s);
        }
        X[(int64_t)d.row * ldx + j] = finish_row(alpha, B[(int64_t)d.row * ldb + j], s, pivot);
    }
}

// ---- wide: one level.  SpSV: the level's units first .. first + count - 1, four lanes each --------------------------
__global__ __launch_bounds__(WIDE_THREADS) void sptrsv_wide_kernel(int64_t first, int64_t count, int lower, const Unit *__restrict__ units,
                                                                   const int32_t *__restrict__ colidx, const double *__restrict__ val,
                                                                   double alpha, const double *b, double *x)
{
    const int64_t t = (int64_t)blockIdx.x * WIDE_THREADS + threadIdx.x;
    const int64_t u = t >> 2;
    solve_row(u < count ? load_unit(units, first + u) : NO_UNIT, (int)(t & 3), lower != 0, colidx, val, alpha, b, x);
}

// SpSM: rows first .. first + rows - 1 of the order, a slot of 1 << wshift lanes each
__global__ __launch_bounds__(WIDE_THREADS) void sptrsm_wide_kernel(int64_t first, int64_t rows, int wshift, int lower,
                                                                   const RowDesc *__restrict__ desc, const int32_t *__restrict__ colidx,
                                                                   const double *__restrict__ val, int64_t nrhs, double alpha,
                                                                   const double *B, int64_t ldb, double *X, int64_t ldx)
{
    const int64_t t = (int64_t)blockIdx.x * WIDE_THREADS + threadIdx.x;
    const int64_t r = t >> wshift;
    if (r >= rows) return;
    solve_row_m(load_desc(desc, first + r), (int)(t & ((1 << wshift) - 1)), 1 << wshift, lower != 0, colidx, val, nrhs, alpha, B, ldb, X, ldx);
}

// ---- chain: levels l0 .. l1 - 1 in one workgroup; a level wider than the workgroup is looped over ------------
__global__ __launch_bounds__(SPTRSV_CHAIN_THREADS) void sptrsv_chain_kernel(int64_t l0, int64_t l1, int lower,
                                                                            const int64_t *__restrict__ level_unit_ptr,
                                                                            const Unit *__restrict__ units,
                                                                            const int32_t *__restrict__ colidx,
                                                                            const double *__restrict__ val, double alpha, const double *b,
                                                                            double *x)
{
    constexpr int PASS = SPTRSV_CHAIN_THREADS / 4; // units of one pass
    const int mine = threadIdx.x >> 2, quad = threadIdx.x & 3;
    // The plan's arrays do not depend on x: the next level's extent and this thread's first unit of it are fetched while
    // the current level is solved, so that behind the barrier only the row's entries and x are waited for.
    int64_t first = level_unit_ptr[l0], end = level_unit_ptr[l0 + 1];
    Unit cur = mine < end - first ? load_unit(units, first + mine) : NO_UNIT;
    for (int64_t l = l0; l < l1; ++l) {
        const int64_t count = end - first, next_end = l + 1 < l1 ? level_unit_ptr[l + 2] : end;
        const Unit next = l + 1 < l1 && mine < next_end - end ? load_unit(units, end + mine) : NO_UNIT;
        solve_row(cur, quad, lower != 0, colidx, val, alpha, b, x);
        for (int64_t u0 = PASS; u0 < count; u0 += PASS) { // the same trip count in every thread
            const int64_t u = u0 + mine;
            solve_row(u < count ? load_unit(units, first + u) : NO_UNIT, quad, lower != 0, colidx, val, alpha, b, x);
        }
        __syncthreads(); // this level's x, stored by this workgroup, is what the next level loads
        first = end, end = next_end, cur = next;
    }
}

__global__ __launch_bounds__(SPTRSV_CHAIN_THREADS) void sptrsm_chain_kernel(int64_t l0, int64_t l1, int wshift, int lower,
                                                                            const int32_t *__restrict__ level_ptr,
                                                                            const RowDesc *__restrict__ desc,
                                                                            const int32_t *__restrict__ colidx,
                                                                            const double *__restrict__ val, int64_t nrhs, double alpha,
                                                                            const double *B, int64_t ldb, double *X, int64_t ldx)
{
    const int slots = SPTRSV_CHAIN_THREADS >> wshift, slot = threadIdx.x >> wshift, lane = threadIdx.x & ((1 << wshift) - 1);
    for (int64_t l = l0; l < l1; ++l) {
        const int64_t first = level_ptr[l], rows = level_ptr[l + 1] - first;
        for (int64_t r = slot; r < rows; r += slots)
            solve_row_m(load_desc(desc, first + r), lane, 1 << wshift, lower != 0, colidx, val, nrhs, alpha, B, ldb, X, ldx);
        __syncthreads();
    }
}

struct Launch {
    int64_t l0, l1; // levels
    bool chain;
};

struct SptrsvPlan {
    int dev = -1, fill = 0, diag = 0, flags = 0;
    int64_t n = 0, nnz = 0, levels = 0, wide = 0, chains = 0, widest = 0, longest = 0, chain_rows = 0;
    size_t bytes = 0;
    const int32_t *rowptr = nullptr, *colidx = nullptr; // the caller's
    DeviceBuffer buf;                                   // units | desc | level_unit_ptr | perm | level_ptr
    Unit *units = nullptr;                              // SpSV: the rows of every level packed into four-lane units
    RowDesc *desc = nullptr;                            // SpSM: the rows by (level, row)
    int64_t *level_unit_ptr = nullptr;
    int32_t *perm = nullptr, *level_ptr = nullptr;
    std::vector<int32_t> h_level_ptr;
    std::vector<int64_t> h_level_unit_ptr;
    std::vector<Launch> launches;
};

inline size_t pad16(size_t b) { return (b + 15) / 16 * 16; }
inline unsigned wide_grid(int64_t lanes) { return (unsigned)((lanes + WIDE_THREADS - 1) / WIDE_THREADS); }
// lanes along the right-hand sides: the least power of two that covers nrhs, a wave at the most
inline int rhs_shift(int64_t nrhs)
{
    int s = 0;
    while (s < 6 && ((int64_t)1 << s) < nrhs) ++s;
    return s;
}

// 0 when the call may run; the plan's device must be current and the structure the one the plan was made for
int call_ok(const SptrsvPlan *p, const int32_t *rowptr, const int32_t *colidx)
{
    if (!p) return SBLAS_E_INVALID;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    if (rowptr != p->rowptr || colidx != p->colidx) return SBLAS_E_INVALID;
    return SBLAS_OK;
}

} // namespace

extern "C" {

int sblas_hip_sptrsv_plan_create(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                                 int fill, int diag, int flags, int64_t chain_rows, void **plan_out, int64_t *bad_row)
{
    if (bad_row) *bad_row = -1;
    if (!plan_out) return SBLAS_E_INVALID;
    *plan_out = nullptr;
    if (n < 0 || nnz < 0 || n > INT_MAX - 64 || nnz > INT_MAX || chain_rows < 0) return SBLAS_E_INVALID;
    if (fill != SBLAS_FILL_LOWER && fill != SBLAS_FILL_UPPER) return SBLAS_E_INVALID;
    if (diag != SBLAS_DIAG_NON_UNIT && diag != SBLAS_DIAG_UNIT) return SBLAS_E_INVALID;
    if (flags != SBLAS_SPTRSV_AUTO && flags != SBLAS_SPTRSV_PER_LEVEL && flags != SBLAS_SPTRSV_CHAIN_ONLY) return SBLAS_E_INVALID;
    if ((n > 0 && !rowptr) || (nnz > 0 && !colidx)) return SBLAS_E_INVALID;
    std::unique_ptr<SptrsvPlan> p(new SptrsvPlan);
    p->dev = resolve_device(dev), p->fill = fill, p->diag = diag, p->flags = flags, p->n = n, p->nnz = nnz;
    p->rowptr = rowptr, p->colidx = colidx;
    p->chain_rows = chain_rows > 0 ? chain_rows : SPTRSV_CHAIN_ROWS;
    if (n == 0) {
        if (nnz != 0) return SBLAS_E_INVALID;
        *plan_out = p.release();
        return SBLAS_OK;
    }
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    hipStream_t s = (hipStream_t)stream;

    // the structure comes to the host once; every check and the whole schedule are host work
    std::vector<int32_t> h_rowptr((size_t)n + 1), h_colidx((size_t)nnz);
    hipError_t e = hipMemcpyAsync(h_rowptr.data(), rowptr, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && nnz > 0) e = hipMemcpyAsync(h_colidx.data(), colidx, (size_t)nnz * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return SBLAS_E_HIP;
    if (h_rowptr[n] != nnz) { // first: the host rule follows rowptr into a colidx of nnz entries
        if (bad_row) *bad_row = n - 1;
        return SBLAS_E_INVALID;
    }
    std::vector<int32_t> level((size_t)n);
    int64_t n_levels = 0;
    const int rc = sblas_sptrsv_levels(n, h_rowptr.data(), h_colidx.data(), fill, diag, level.data(), &n_levels, bad_row);
    if (rc != SBLAS_OK) return rc;
    p->levels = n_levels;

    // rows by (level, row): a counting sort, stable in the row
    std::vector<int32_t> &lp = p->h_level_ptr;
    lp.assign((size_t)n_levels + 1, 0);
    for (int64_t i = 0; i < n; ++i) ++lp[(size_t)level[i] + 1];
    std::vector<int64_t> widths((size_t)n_levels);
    for (int64_t l = 0; l < n_levels; ++l) {
        widths[l] = lp[l + 1];
        p->widest = widths[l] > p->widest ? widths[l] : p->widest;
        lp[l + 1] += lp[l];
    }
    std::vector<int32_t> perm((size_t)n), fillpos(lp.begin(), lp.end() - 1);
    std::vector<RowDesc> desc((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int32_t k = fillpos[level[i]]++;
        perm[k] = (int32_t)i;
        int32_t dpos = -1;
        if (diag == SBLAS_DIAG_NON_UNIT)
            for (int32_t q = h_rowptr[i]; q < h_rowptr[i + 1]; ++q)
                if (h_colidx[q] == i) dpos = q;
        desc[k] = RowDesc{(int32_t)i, h_rowptr[i], h_rowptr[i + 1], dpos};
        const int64_t len = (int64_t)h_rowptr[i + 1] - h_rowptr[i];
        p->longest = len > p->longest ? len : p->longest;
    }
    // SpSV's lanes: every level packs its rows, in order, into four-lane units; a row of G lanes starts on a multiple of
    // G lanes of its level (its butterfly stays inside one DPP row, or is one wave), and padding units fill the gaps
    std::vector<Unit> units;
    units.reserve((size_t)n + (size_t)n / 4);
    std::vector<int64_t> &up = p->h_level_unit_ptr;
    up.assign((size_t)n_levels + 1, 0);
    for (int64_t l = 0; l < n_levels; ++l) {
        up[l] = (int64_t)units.size();
        for (int32_t k = lp[l]; k < lp[l + 1]; ++k) {
            const RowDesc &d = desc[k];
            const size_t per_row = (size_t)1 << (sptrsv_group_shift((int64_t)d.end - d.beg) - 2); // units of this row
            while ((units.size() - (size_t)up[l]) % per_row) units.push_back(NO_UNIT);
            units.push_back(Unit{d.row, d.beg, d.end, d.diag});
            for (size_t q = 1; q < per_row; ++q) units.push_back(Unit{d.row, d.beg, d.end, -2 - (int32_t)q});
        }
    }
    up[n_levels] = (int64_t)units.size();

    // the launches
    std::vector<uint8_t> kind((size_t)n_levels);
    std::vector<int64_t> lfirst((size_t)n_levels + 1);
    int64_t n_launches = 0;
    if (sblas_sptrsv_schedule(n_levels, widths.data(), flags, chain_rows, kind.data(), lfirst.data(), &n_launches) != SBLAS_OK)
        return SBLAS_E_INVALID;
    for (int64_t q = 0; q < n_launches; ++q) {
        const bool chain = kind[q] == SBLAS_SPTRSV_LAUNCH_CHAIN;
        p->launches.push_back(Launch{lfirst[q], lfirst[q + 1], chain});
        ++(chain ? p->chains : p->wide);
    }

    const size_t o_desc = units.size() * sizeof(Unit), o_up = o_desc + (size_t)n * sizeof(RowDesc);
    const size_t o_perm = o_up + pad16(((size_t)n_levels + 1) * 8), o_lp = o_perm + pad16((size_t)n * 4);
    const size_t total = o_lp + pad16(((size_t)n_levels + 1) * 4);
    if (p->buf.alloc(p->dev, total) != hipSuccess) return SBLAS_E_HIP;
    p->bytes = total;
    p->units = p->buf.at<Unit>(), p->desc = p->buf.at<RowDesc>(o_desc), p->level_unit_ptr = p->buf.at<int64_t>(o_up);
    p->perm = p->buf.at<int32_t>(o_perm), p->level_ptr = p->buf.at<int32_t>(o_lp);
    e = hipMemcpyAsync(p->units, units.data(), units.size() * sizeof(Unit), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(p->desc, desc.data(), (size_t)n * sizeof(RowDesc), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(p->level_unit_ptr, up.data(), ((size_t)n_levels + 1) * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(p->perm, perm.data(), (size_t)n * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(p->level_ptr, lp.data(), ((size_t)n_levels + 1) * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s); // the host vectors are read until here
    if (e != hipSuccess) return SBLAS_E_HIP;
    *plan_out = p.release();
    return SBLAS_OK;
}

int sblas_hip_sptrsv_plan_info(const void *plan, int64_t out[12])
{
    if (!plan || !out) return SBLAS_E_INVALID;
    const SptrsvPlan *p = static_cast<const SptrsvPlan *>(plan);
    out[0] = p->n, out[1] = p->nnz, out[2] = p->fill, out[3] = p->diag, out[4] = p->levels, out[5] = (int64_t)p->launches.size();
    out[6] = p->wide, out[7] = p->chains, out[8] = p->widest, out[9] = p->longest, out[10] = (int64_t)p->bytes, out[11] = p->flags;
    return SBLAS_OK;
}

int sblas_hip_sptrsv_plan_speaks_for(const void *plan, int dev, const int32_t *rowptr, const int32_t *colidx)
{
    const SptrsvPlan *p = static_cast<const SptrsvPlan *>(plan);
    if (!p || p->dev != resolve_device(dev)) return SBLAS_E_INVALID;
    return rowptr == p->rowptr && colidx == p->colidx ? SBLAS_OK : SBLAS_E_INVALID;
}

int sblas_hip_sptrsv_plan_order(const void *plan, const int32_t **perm, const int32_t **level_ptr)
{
    if (!plan) return SBLAS_E_INVALID;
    const SptrsvPlan *p = static_cast<const SptrsvPlan *>(plan);
    if (perm) *perm = p->perm;
    if (level_ptr) *level_ptr = p->level_ptr;
    return SBLAS_OK;
}

int sblas_hip_sptrsv_plan_destroy(void *plan)
{
    delete static_cast<SptrsvPlan *>(plan);
    return SBLAS_OK;
}

int sblas_hip_sptrsv_f64_i32_planned(const void *plan, void *stream, const int32_t *rowptr, const int32_t *colidx, const double *val,
                                     double alpha, const double *b, double *x)
{
    const SptrsvPlan *p = static_cast<const SptrsvPlan *>(plan);
    const int rc = call_ok(p, rowptr, colidx);
    if (rc != SBLAS_OK) return rc;
    if (p->n == 0) return SBLAS_OK;
    if (!b || !x || (p->nnz > 0 && !val)) return SBLAS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int lower = p->fill == SBLAS_FILL_LOWER;
    for (const Launch &q : p->launches) {
        if (q.chain) {
            sptrsv_chain_kernel<<<1, SPTRSV_CHAIN_THREADS, 0, s>>>(q.l0, q.l1, lower, p->level_unit_ptr, p->units, colidx, val, alpha, b, x);
        } else {
            const int64_t first = p->h_level_unit_ptr[q.l0], count = p->h_level_unit_ptr[q.l1] - first;
            sptrsv_wide_kernel<<<wide_grid(4 * count), WIDE_THREADS, 0, s>>>(first, count, lower, p->units, colidx, val, alpha, b, x);
        }
    }
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_sptrsm_f64_i32_planned(const void *plan, void *stream, const int32_t *rowptr, const int32_t *colidx, const double *val,
                                     int64_t nrhs, double alpha, const double *B, int64_t ldb, double *X, int64_t ldx)
{
    const SptrsvPlan *p = static_cast<const SptrsvPlan *>(plan);
    const int rc = call_ok(p, rowptr, colidx);
    if (rc != SBLAS_OK) return rc;
    if (nrhs < 0 || ldb < nrhs || ldx < nrhs) return SBLAS_E_INVALID;
    if (p->n == 0 || nrhs == 0) return SBLAS_OK;
    if (!B || !X || (p->nnz > 0 && !val)) return SBLAS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int lower = p->fill == SBLAS_FILL_LOWER, ws = rhs_shift(nrhs);
    for (const Launch &q : p->launches) {
        if (q.chain) {
            sptrsm_chain_kernel<<<1, SPTRSV_CHAIN_THREADS, 0, s>>>(q.l0, q.l1, ws, lower, p->level_ptr, p->desc, colidx, val, nrhs, alpha, B, ldb, X, ldx);
        } else {
            const int64_t first = p->h_level_ptr[q.l0], rows = p->h_level_ptr[q.l1] - first;
            sptrsm_wide_kernel<<<wide_grid(rows << ws), WIDE_THREADS, 0, s>>>(first, rows, ws, lower, p->desc, colidx, val, nrhs, alpha, B, ldb, X, ldx);
        }
    }
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

} // extern "C"
