// sptrsv.hip -- sparse triangular solves on a level-scheduled plan: T x = alpha b (SpSV) and
// T X = alpha B for nrhs right-hand sides (SpSM), T the lower or upper triangle of a square CSR matrix.
//
// The plan sorts the rows by (level, row) once (the host rules: sptrsv_plan.cpp, level_plan.h); a solve is then a fixed
// sequence of wide and chain launches.  The two walks, and why x stored before a chain launch's barrier is what is
// loaded behind it, are in level_kernels.h.  x and b are not __restrict__: they may be the same array, and x is read and
// written in one launch.
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
#include "level_kernels.h"
#include "rowwise.h"
#include "sptrsv.h"
#include "unit_row.h"

using namespace sblas;

namespace {

constexpr int WIDE_THREADS = 256;

// a row as the SpSM kernels meet it, in (level, row) order: one 16-byte load (load_unit)
struct RowDesc {
    int32_t row, beg, end, diag; // diag: position of the stored diagonal in val, -1 under SBLAS_DIAG_UNIT
};

__device__ __forceinline__ double finish_row(double alpha, double bi, double sum, double pivot)
{
#pragma clang fp contract(off) // three roundings, on every path: alpha * b, the subtraction, the division
    const double t = alpha * bi;
    return (t - sum) / pivot;
}

// SpSV's unit record (level_plan.h: four lanes of a launch; a pad has row = -1).  tag: in a row's first unit the position
// of the stored diagonal in val (-1 under SBLAS_DIAG_UNIT); in its unit number s > 0, -2 - s.
struct Unit {
    int32_t row, beg, end, tag;
};
constexpr Unit NO_UNIT{-1, 0, 0, -1};

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
    const double sum = group_fold(s, gs);
    if (writer) x[u.row] = finish_row(alpha, bi, sum, pivot);
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
    solve_row(wide_unit<WIDE_THREADS>(first, count, units, NO_UNIT), threadIdx.x & 3, lower != 0, colidx, val, alpha, b, x);
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
    solve_row_m(load_unit(desc, first + r), (int)(t & ((1 << wshift) - 1)), 1 << wshift, lower != 0, colidx, val, nrhs, alpha, B, ldb, X, ldx);
}

// ---- chain: levels l0 .. l1 - 1 in one workgroup; a level wider than the workgroup is looped over ------------
__global__ __launch_bounds__(SPTRSV_CHAIN_THREADS) void sptrsv_chain_kernel(int64_t l0, int64_t l1, int lower,
                                                                            const int64_t *__restrict__ level_unit_ptr,
                                                                            const Unit *__restrict__ units,
                                                                            const int32_t *__restrict__ colidx,
                                                                            const double *__restrict__ val, double alpha, const double *b,
                                                                            double *x)
{
    chain_walk<SPTRSV_CHAIN_THREADS>(l0, l1, level_unit_ptr, units, NO_UNIT,
                                     [&](const Unit u) { solve_row(u, threadIdx.x & 3, lower != 0, colidx, val, alpha, b, x); });
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
            solve_row_m(load_unit(desc, first + r), lane, 1 << wshift, lower != 0, colidx, val, nrhs, alpha, B, ldb, X, ldx);
        __syncthreads();
    }
}

struct SptrsvPlan : LevelPlan { // buf: units | desc | level_unit_ptr | perm | level_ptr
    int fill = 0, diag = 0;
    Unit *units = nullptr;   // SpSV: the rows of every level packed into four-lane units
    RowDesc *desc = nullptr; // SpSM: the rows by (level, row)
    int32_t *perm = nullptr, *level_ptr = nullptr;
    std::vector<int32_t> h_level_ptr;
};

// lanes along the right-hand sides: the least power of two that covers nrhs, a wave at the most
inline int rhs_shift(int64_t nrhs)
{
    int s = 0;
    while (s < 6 && ((int64_t)1 << s) < nrhs) ++s;
    return s;
}

} // namespace

#include "sptrsm_tile_kernels.h" // solve_row() over a tile of eight columns, and its two kernels

extern "C" {

int sblas_hip_sptrsv_plan_create(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                                 int fill, int diag, int flags, int64_t chain_rows, void **plan_out, int64_t *bad_row)
{
    std::unique_ptr<SptrsvPlan> p(new SptrsvPlan);
    if (!level_plan_begin(*p, dev, n, nnz, rowptr, colidx, flags, chain_rows, SPTRSV_CHAIN_ROWS, plan_out, bad_row)) return SBLAS_E_INVALID;
    if (fill != SBLAS_FILL_LOWER && fill != SBLAS_FILL_UPPER) return SBLAS_E_INVALID;
    if (diag != SBLAS_DIAG_NON_UNIT && diag != SBLAS_DIAG_UNIT) return SBLAS_E_INVALID;
    p->fill = fill, p->diag = diag;
    if (n == 0) {
        *plan_out = p.release();
        return SBLAS_OK;
    }
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int32_t> h_rowptr, h_colidx, level((size_t)n);
    int rc = fetch_structure(s, n, nnz, rowptr, colidx, h_rowptr, h_colidx, bad_row);
    if (rc != SBLAS_OK) return rc;
    rc = sblas_sptrsv_levels(n, h_rowptr.data(), h_colidx.data(), fill, diag, level.data(), &p->levels, bad_row);
    if (rc != SBLAS_OK) return rc;

    std::vector<int32_t> dpos((size_t)n, -1); // every row's stored diagonal
    for (int64_t i = 0; i < n; ++i) {
        if (diag == SBLAS_DIAG_NON_UNIT)
            for (int32_t q = h_rowptr[i]; q < h_rowptr[i + 1]; ++q)
                if (h_colidx[q] == i) dpos[i] = q;
        const int64_t len = (int64_t)h_rowptr[i + 1] - h_rowptr[i];
        p->longest = len > p->longest ? len : p->longest;
    }
    LevelOrder o;
    std::vector<Unit> units; // SpSV's lanes
    const auto unit_of = [&](int32_t i, int32_t q) { return Unit{i, h_rowptr[i], h_rowptr[i + 1], q ? -2 - q : dpos[i]}; };
    level_pack(n, h_rowptr.data(), level.data(), p->levels, unit_of, NO_UNIT, o, units);
    std::vector<RowDesc> desc((size_t)n); // SpSM's rows
    for (int64_t k = 0; k < n; ++k) {
        const int32_t i = o.perm[k];
        desc[k] = RowDesc{i, h_rowptr[i], h_rowptr[i + 1], dpos[i]};
    }
    if (level_launches(o.widths, flags, p->chain_rows, p->sched) != SBLAS_OK) return SBLAS_E_INVALID;

    Segment seg[5] = {Segment(units), Segment(desc), Segment(o.level_unit_ptr), Segment(o.perm), Segment(o.level_ptr)};
    if (upload_segments(p->buf, p->dev, s, seg, 5, &p->bytes) != hipSuccess) return SBLAS_E_HIP;
    p->units = p->buf.at<Unit>(), p->desc = p->buf.at<RowDesc>(seg[1].offset), p->level_unit_ptr = p->buf.at<int64_t>(seg[2].offset);
    p->perm = p->buf.at<int32_t>(seg[3].offset), p->level_ptr = p->buf.at<int32_t>(seg[4].offset);
    p->h_level_unit_ptr = std::move(o.level_unit_ptr), p->h_level_ptr = std::move(o.level_ptr);
    *plan_out = p.release();
    return SBLAS_OK;
}

int sblas_hip_sptrsv_plan_info(const void *plan, int64_t out[12])
{
    if (!plan || !out) return SBLAS_E_INVALID;
    const SptrsvPlan *p = static_cast<const SptrsvPlan *>(plan);
    out[0] = p->n, out[1] = p->nnz, out[2] = p->fill, out[3] = p->diag, out[4] = p->levels, out[5] = (int64_t)p->sched.launches.size();
    out[6] = p->sched.wide, out[7] = p->sched.chains, out[8] = p->sched.widest, out[9] = p->longest, out[10] = (int64_t)p->bytes;
    out[11] = p->flags;
    return SBLAS_OK;
}

int sblas_hip_sptrsv_plan_speaks_for(const void *plan, int dev, const int32_t *rowptr, const int32_t *colidx)
{
    return level_plan_speaks_for(static_cast<const SptrsvPlan *>(plan), dev, rowptr, colidx);
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
    const int rc = level_plan_speaks_for(p, -1, rowptr, colidx);
    if (rc != SBLAS_OK) return rc;
    if (p->n == 0) return SBLAS_OK;
    if (!b || !x || (p->nnz > 0 && !val)) return SBLAS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int lower = p->fill == SBLAS_FILL_LOWER;
    for (const Launch &q : p->sched.launches) {
        if (q.chain) {
            sptrsv_chain_kernel<<<1, SPTRSV_CHAIN_THREADS, 0, s>>>(q.l0, q.l1, lower, p->level_unit_ptr, p->units, colidx, val, alpha, b, x);
        } else {
            const int64_t first = p->h_level_unit_ptr[q.l0], count = p->h_level_unit_ptr[q.l1] - first;
            sptrsv_wide_kernel<<<wide_grid(4 * count, WIDE_THREADS), WIDE_THREADS, 0, s>>>(first, count, lower, p->units, colidx, val, alpha, b, x);
        }
    }
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_sptrsm_f64_i32_planned(const void *plan, void *stream, const int32_t *rowptr, const int32_t *colidx, const double *val,
                                     int64_t nrhs, double alpha, const double *B, int64_t ldb, double *X, int64_t ldx)
{
    const SptrsvPlan *p = static_cast<const SptrsvPlan *>(plan);
    const int rc = level_plan_speaks_for(p, -1, rowptr, colidx);
    if (rc != SBLAS_OK) return rc;
    if (nrhs < 0 || ldb < nrhs || ldx < nrhs) return SBLAS_E_INVALID;
    if (p->n == 0 || nrhs == 0) return SBLAS_OK;
    if (!B || !X || (p->nnz > 0 && !val)) return SBLAS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int lower = p->fill == SBLAS_FILL_LOWER, ws = rhs_shift(nrhs);
    for (const Launch &q : p->sched.launches) {
        if (q.chain) {
            sptrsm_chain_kernel<<<1, SPTRSV_CHAIN_THREADS, 0, s>>>(q.l0, q.l1, ws, lower, p->level_ptr, p->desc, colidx, val, nrhs, alpha, B, ldb, X, ldx);
        } else {
            const int64_t first = p->h_level_ptr[q.l0], rows = p->h_level_ptr[q.l1] - first;
            sptrsm_wide_kernel<<<wide_grid(rows << ws, WIDE_THREADS), WIDE_THREADS, 0, s>>>(first, rows, ws, lower, p->desc, colidx, val, nrhs, alpha, B, ldb, X, ldx);
        }
    }
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

// The tiled SpSM: the single solve's launches, each widened by ceil(nrhs / 8) tiles.
int sblas_hip_sptrsm_tiled_f64_i32_planned(const void *plan, void *stream, const int32_t *rowptr, const int32_t *colidx, const double *val,
                                           int64_t nrhs, double alpha, const double *B, int64_t ldb, double *X, int64_t ldx)
{
    const SptrsvPlan *p = static_cast<const SptrsvPlan *>(plan);
    const int rc = level_plan_speaks_for(p, -1, rowptr, colidx);
    if (rc != SBLAS_OK) return rc;
    if (nrhs < 0 || ldb < nrhs || ldx < nrhs) return SBLAS_E_INVALID;
    if (p->n == 0 || nrhs == 0) return SBLAS_OK;
    if (!B || !X || (p->nnz > 0 && !val)) return SBLAS_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(B) | reinterpret_cast<uintptr_t>(X)) & 7u) return SBLAS_E_INVALID;
    // every grid is known from the plan: an nrhs whose widest launch would not fit is refused before anything is launched
    for (const Launch &q : p->sched.launches)
        if (tile_grid(q.chain ? 1 : unit_blocks(p->h_level_unit_ptr[q.l1] - p->h_level_unit_ptr[q.l0], SPTRSM_UNITS_PER_BLOCK), nrhs) < 0)
            return SBLAS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const TileSolveArgs a{p->fill == SBLAS_FILL_LOWER, nrhs, p->units, colidx, val, alpha, B, ldb, X, ldx};
    const bool wide = wide16(B, ldb) && wide16(X, ldx);
    const unsigned ntiles = (unsigned)tiles(nrhs);
    for (const Launch &q : p->sched.launches) {
        if (q.chain) {
            if (wide) sptrsm_tile_chain_kernel<true><<<ntiles, SPTRSV_CHAIN_THREADS, 0, s>>>(q.l0, q.l1, p->level_unit_ptr, a);
            else sptrsm_tile_chain_kernel<false><<<ntiles, SPTRSV_CHAIN_THREADS, 0, s>>>(q.l0, q.l1, p->level_unit_ptr, a);
        } else {
            const int64_t first = p->h_level_unit_ptr[q.l0], count = p->h_level_unit_ptr[q.l1] - first;
            const int64_t blocks = unit_blocks(count, SPTRSM_UNITS_PER_BLOCK);
            const unsigned grid = (unsigned)tile_grid(blocks, nrhs);
            if (wide) sptrsm_tile_wide_kernel<true><<<grid, SPTRSM_WIDE_THREADS, 0, s>>>(first, count, blocks, a);
            else sptrsm_tile_wide_kernel<false><<<grid, SPTRSM_WIDE_THREADS, 0, s>>>(first, count, blocks, a);
        }
    }
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

} // extern "C"
