// ilu0.hip -- ILU(0) of a square CSR matrix on a level-scheduled plan, factored on the device:
// lu = ILU0(A) on A's own pattern, the strictly-lower entries of the unit-lower L and the diagonal and upper entries of U
// in one CSR, which is what two triangular-solve plans (lower / unit, upper) on (rowptr, colidx, lu) consume.
//
// The schedule is the lower solve's: row i needs the finished rows k < i it stores an entry for.  A factorisation is a
// fixed sequence of wide and chain launches, as a solve is, on the same walks (level_kernels.h).
//
// factor_row() is the one expression of a row, shared by both kernels.  A row of p stored entries belongs to G(p) lanes
// (the solves' G).  Two tiers:
//   LDS   p <= ILU0_LDS_MAX: the group copies the row (columns and values) into its slice of LDS, walks the entries left
//         of the diagonal in order, and for each such column k strides over row k's upper part in global memory, each lane
//         searching its column in the LDS copy and updating the LDS value; then the row is stored.
//   long  a longer row belongs to a whole wave and works in lu itself, in the gather form: lane l owns the entries l,
//         l + 64, ... of row i and is the only thread that ever touches them, the multiplier travels by a lane broadcast,
//         and each lane searches row k for its own columns.  No memory is shared between lanes at all.
//
// Ordering inside a row (LDS tier).  Step k + 1 reads LDS values that other lanes of the group wrote in step k.  A group
// lies inside one wave and so does its slice: the wave issues its LDS instructions in program order and the LDS unit
// completes them in order, so only the compiler could break the order.  step_fence() -- a wavefront-scope release, a
// wave barrier and a wavefront-scope acquire -- forbids that; it emits no instruction of its own beyond a wait.  Lanes of a
// group have the same trip counts in every loop that holds a fence, so they meet it together.
//
// Visibility of row k.  Its values are read from lu, never from val, with plain global loads, and were stored with
// plain global stores by an earlier launch (the kernel boundary orders everything) or by this workgroup before the
// barrier of the chain walk, whose argument is in level_kernels.h.  lu and val are not __restrict__: they may be the same
// array, and lu is read and written in one launch, which also keeps it off the scalar path.
//
// Results contract: each entry receives its updates one after another in ascending k, each as a rounded product and a
// rounded difference; no sum is folded across lanes.  The bits of lu are a function of val and the pattern alone.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <memory>
#include <vector>
#include "../../include/sblas_hip.h"
#include "ilu0.h"
#include "level_kernels.h"

using namespace sblas;

namespace {

constexpr Ilu0Unit NO_UNIT{-1, 0, 0, 0};

__device__ __forceinline__ double sub_prod(double w, double l, double u)
{
#pragma clang fp contract(off) // two roundings, on every path: the product, then the difference
    const double t = l * u;
    return w - t;
}

// orders the LDS traffic of one wave's lanes: what a lane wrote before is what another lane of the wave reads after
__device__ __forceinline__ void step_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Row u.row of lu.  lcol / lval: the workgroup's LDS, ILU0_LDS_PER_LANE entries a thread.  The lane's place in its row is
// its place in the workgroup modulo G: the plan aligns a row to G lanes of its level, and a workgroup (or a pass of the
// chain workgroup) starts on a multiple of 64 lanes of the level.
__device__ __forceinline__ void factor_row(const Ilu0Unit u, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                                           const int32_t *__restrict__ diag_pos, const double *val, double *lu, int32_t *lcol,
                                           double *lval)
{
    if (u.row < 0) return; // whole groups leave together: nothing below crosses a group
    const int p = u.end - u.beg, nl = u.diag - u.beg;
    const int G = 1 << sptrsv_group_shift(p), ln = (int)threadIdx.x & (G - 1);
    if (p <= ILU0_LDS_MAX) {
        int32_t *c = lcol + ((int)threadIdx.x - ln) * ILU0_LDS_PER_LANE;
        double *w = lval + ((int)threadIdx.x - ln) * ILU0_LDS_PER_LANE;
        step_fence(); // the slice's last row was read out by other lanes
        for (int e = ln; e < p; e += G) c[e] = colidx[(int64_t)u.beg + e], w[e] = val[(int64_t)u.beg + e];
        // Which rows k the row meets, and where their upper parts lie, depends on no value: step q + 1's are fetched
        // while step q runs, so that a step waits for row k's entries alone.
        step_fence(); // the copy
        int k_next = nl > 0 ? c[0] : u.row;
        int64_t dk_next = diag_pos[k_next], kend_next = rowptr[k_next + 1];
        for (int q = 0; q < nl; ++q) {
            step_fence(); // step q - 1's updates
            const double wq = w[q];
            const int64_t dk = dk_next, kend = kend_next;
            k_next = q + 1 < nl ? c[q + 1] : u.row;
            dk_next = diag_pos[k_next], kend_next = rowptr[k_next + 1];
            // every lane forms the multiplier from the same two numbers (the same bits as if its owner alone did, and
            // no exchange); one lane stores it.  Nothing reads w[q] again before the row is stored.
            const double l = wq / lu[dk];
            if (ln == 0) w[q] = l;
            for (int64_t f = dk + 1 + ln; f < kend; f += G) {
                const int j = colidx[f];
                const double ukj = lu[f];
                int lo = q + 1, hi = p; // columns ascend: j > k lies right of q
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (c[mid] < j) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < p && c[lo] == j) w[lo] = sub_prod(w[lo], l, ukj); // row k's columns differ: one lane an entry
            }
        }
        step_fence();
        for (int e = ln; e < p; e += G) lu[(int64_t)u.beg + e] = w[e];
        return;
    }
    // long tier: a whole wave (G = 64), every entry private to the lane that owns it
    for (int64_t e = (int64_t)u.beg + ln; e < u.end; e += 64) lu[e] = val[e]; // in place: onto itself
    for (int q = 0; q < nl; ++q) {
        const int owner = q & 63;
        const int k = colidx[(int64_t)u.beg + q];
        const int64_t dk = diag_pos[k], kend = rowptr[k + 1];
        double l = 0.0;
        if (ln == owner) {
            l = lu[(int64_t)u.beg + q] / lu[dk];
            lu[(int64_t)u.beg + q] = l;
        }
        l = __shfl(l, owner);
        // the lane's own entries right of q
        const int t0 = q + 1 <= ln ? 0 : (q + 1 - ln + 63) / 64;
        for (int64_t e = (int64_t)u.beg + ln + 64 * (int64_t)t0; e < u.end; e += 64) {
            const int j = colidx[e];
            int64_t lo = dk + 1, hi = kend;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (colidx[mid] < j) lo = mid + 1;
                else hi = mid;
            }
            if (lo < kend && colidx[lo] == j) lu[e] = sub_prod(lu[e], l, lu[lo]);
        }
    }
}

// ---- wide: one level, its units first .. first + count - 1, four lanes each ------------------------------------------
__global__ __launch_bounds__(ILU0_WIDE_THREADS) void ilu0_wide_kernel(int64_t first, int64_t count, const Ilu0Unit *__restrict__ units,
                                                                      const int32_t *__restrict__ rowptr,
                                                                      const int32_t *__restrict__ colidx,
                                                                      const int32_t *__restrict__ diag_pos, const double *val, double *lu)
{
    __shared__ int32_t lcol[ILU0_WIDE_THREADS * ILU0_LDS_PER_LANE];
    __shared__ double lval[ILU0_WIDE_THREADS * ILU0_LDS_PER_LANE];
    factor_row(wide_unit<ILU0_WIDE_THREADS>(first, count, units, NO_UNIT), rowptr, colidx, diag_pos, val, lu, lcol, lval);
}

// ---- chain: levels l0 .. l1 - 1 in one workgroup; a level wider than the workgroup is looped over --------------------
__global__ __launch_bounds__(ILU0_CHAIN_THREADS) void ilu0_chain_kernel(int64_t l0, int64_t l1, const int64_t *__restrict__ level_unit_ptr,
                                                                        const Ilu0Unit *__restrict__ units,
                                                                        const int32_t *__restrict__ rowptr,
                                                                        const int32_t *__restrict__ colidx,
                                                                        const int32_t *__restrict__ diag_pos, const double *val,
                                                                        double *lu)
{
    __shared__ int32_t lcol[ILU0_CHAIN_THREADS * ILU0_LDS_PER_LANE];
    __shared__ double lval[ILU0_CHAIN_THREADS * ILU0_LDS_PER_LANE];
    chain_walk<ILU0_CHAIN_THREADS>(l0, l1, level_unit_ptr, units, NO_UNIT,
                                   [&](const Ilu0Unit u) { factor_row(u, rowptr, colidx, diag_pos, val, lu, lcol, lval); });
}

struct Ilu0Plan : LevelPlan { // buf: units | level_unit_ptr | diag_pos
    int64_t long_rows = 0;
    Ilu0Unit *units = nullptr;
    int32_t *diag_pos = nullptr;
};

} // namespace

extern "C" {

int sblas_hip_ilu0_plan_create(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx, int flags,
                               int64_t chain_rows, void **plan_out, int64_t *bad_row)
{
    std::unique_ptr<Ilu0Plan> p(new Ilu0Plan);
    if (!level_plan_begin(*p, dev, n, nnz, rowptr, colidx, flags, chain_rows, ILU0_CHAIN_ROWS, plan_out, bad_row)) return SBLAS_E_INVALID;
    if (n == 0) {
        *plan_out = p.release();
        return SBLAS_OK;
    }
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int32_t> h_rowptr, h_colidx, dpos((size_t)n), level((size_t)n);
    int rc = fetch_structure(s, n, nnz, rowptr, colidx, h_rowptr, h_colidx, bad_row);
    if (rc != SBLAS_OK) return rc;
    rc = sblas_ilu0_check(n, h_rowptr.data(), h_colidx.data(), dpos.data(), bad_row);
    if (rc != SBLAS_OK) return rc;
    rc = sblas_sptrsv_levels(n, h_rowptr.data(), h_colidx.data(), SBLAS_FILL_LOWER, SBLAS_DIAG_NON_UNIT, level.data(), &p->levels, bad_row);
    if (rc != SBLAS_OK) return rc;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = (int64_t)h_rowptr[i + 1] - h_rowptr[i];
        p->longest = len > p->longest ? len : p->longest;
        p->long_rows += len > ILU0_LDS_MAX;
    }
    LevelOrder o;
    std::vector<Ilu0Unit> units; // every unit of a row carries the row's record
    const auto unit_of = [&](int32_t i, int32_t) { return Ilu0Unit{i, h_rowptr[i], dpos[i], h_rowptr[i + 1]}; };
    level_pack(n, h_rowptr.data(), level.data(), p->levels, unit_of, NO_UNIT, o, units);
    if (level_launches(o.widths, flags, p->chain_rows, p->sched) != SBLAS_OK) return SBLAS_E_INVALID;

    Segment seg[3] = {Segment(units), Segment(o.level_unit_ptr), Segment(dpos)};
    if (upload_segments(p->buf, p->dev, s, seg, 3, &p->bytes) != hipSuccess) return SBLAS_E_HIP;
    p->units = p->buf.at<Ilu0Unit>(), p->level_unit_ptr = p->buf.at<int64_t>(seg[1].offset), p->diag_pos = p->buf.at<int32_t>(seg[2].offset);
    p->h_level_unit_ptr = std::move(o.level_unit_ptr);
    *plan_out = p.release();
    return SBLAS_OK;
}

int sblas_hip_ilu0_plan_info(const void *plan, int64_t out[12])
{
    if (!plan || !out) return SBLAS_E_INVALID;
    const Ilu0Plan *p = static_cast<const Ilu0Plan *>(plan);
    out[0] = p->n, out[1] = p->nnz, out[2] = p->levels, out[3] = (int64_t)p->sched.launches.size(), out[4] = p->sched.wide;
    out[5] = p->sched.chains, out[6] = p->sched.widest, out[7] = p->longest, out[8] = p->long_rows, out[9] = (int64_t)p->bytes;
    out[10] = p->flags, out[11] = p->chain_rows;
    return SBLAS_OK;
}

int sblas_hip_ilu0_plan_diag(const void *plan, const int32_t **diag_pos)
{
    if (!plan || !diag_pos) return SBLAS_E_INVALID;
    *diag_pos = static_cast<const Ilu0Plan *>(plan)->diag_pos;
    return SBLAS_OK;
}

int sblas_hip_ilu0_plan_destroy(void *plan)
{
    delete static_cast<Ilu0Plan *>(plan);
    return SBLAS_OK;
}

int sblas_hip_ilu0_f64_i32_planned(const void *plan, void *stream, const int32_t *rowptr, const int32_t *colidx, const double *val,
                                   double *lu)
{
    const Ilu0Plan *p = static_cast<const Ilu0Plan *>(plan);
    const int rc = level_plan_speaks_for(p, -1, rowptr, colidx);
    if (rc != SBLAS_OK) return rc;
    if (p->n == 0) return SBLAS_OK;
    if (!val || !lu) return SBLAS_E_INVALID; // n > 0: every row stores its diagonal
    hipStream_t s = (hipStream_t)stream;
    for (const Launch &q : p->sched.launches) {
        if (q.chain) {
            ilu0_chain_kernel<<<1, ILU0_CHAIN_THREADS, 0, s>>>(q.l0, q.l1, p->level_unit_ptr, p->units, rowptr, colidx, p->diag_pos, val, lu);
        } else {
            const int64_t first = p->h_level_unit_ptr[q.l0], count = p->h_level_unit_ptr[q.l1] - first;
            ilu0_wide_kernel<<<wide_grid(4 * count, ILU0_WIDE_THREADS), ILU0_WIDE_THREADS, 0, s>>>(first, count, p->units, rowptr, colidx, p->diag_pos, val, lu);
        }
    }
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

} // extern "C"
