// ilu0.hip -- ILU(0) of a square CSR matrix on a level-scheduled plan, factored on the device:
// lu = ILU0(A) on A's own pattern, the strictly-lower entries of the unit-lower L and the diagonal and upper entries of U
// in one CSR, which is what two triangular-solve plans (lower / unit, upper) on (rowptr, colidx, lu) consume.
//
// The schedule is the lower solve's: row i needs the finished rows k < i it stores an entry for.  A factorisation is a
// fixed sequence of launches of two kernels, as a solve is:
//   wide   one level a launch; the level's rows, in ascending row order, spread over the grid;
//   chain  one workgroup walks a run of consecutive levels with __syncthreads() between them.
// Nothing waits across workgroups: no flag polling, no cooperative launch, no grid barrier, no atomics.  The only
// synchronisation is the kernel boundary and __syncthreads(), and every loop's trip count comes from the structure.
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
// barrier.  __syncthreads() is a workgroup-scope release and acquire: every wave waits for its stores (s_waitcnt
// vmcnt(0)) before it arrives, and no load of lu for a later level is issued before it leaves (what is fetched ahead of
// the barrier is plan data, which no kernel writes).  The waves of one workgroup run on one CU and share its vector L1,
// which is write-through and sees the CU's own stores; the hazard of a stale L1 line exists only between CUs, and no
// other workgroup runs in a chain launch.  lu and val are not __restrict__: they may be the same array, and lu is read
// and written in one launch, which also keeps it off the scalar path.
//
// Results contract: each entry receives its updates one after another in ascending k, each as a rounded product and a
// rounded difference; no sum is folded across lanes.  The bits of lu are a function of val and the pattern alone.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <memory>
#include <vector>
#include "../../include/sblas_hip.h"
#include "capi_util.h"
#include "ilu0.h"

using namespace sblas;

namespace {

constexpr Ilu0Unit NO_UNIT{-1, 0, 0, 0};

__device__ __forceinline__ Ilu0Unit load_unit(const Ilu0Unit *__restrict__ units, int64_t u)
{
    const int4 v = *reinterpret_cast<const int4 *>(units + u);
    return Ilu0Unit{v.x, v.y, v.z, v.w};
}

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
    const int64_t un = ((int64_t)blockIdx.x * ILU0_WIDE_THREADS + threadIdx.x) >> 2;
    factor_row(un < count ? load_unit(units, first + un) : NO_UNIT, rowptr, colidx, diag_pos, val, lu, lcol, lval);
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
    constexpr int PASS = ILU0_CHAIN_THREADS / 4; // units of one pass
    const int mine = threadIdx.x >> 2;
    // The plan's arrays do not depend on lu: the next level's extent and this thread's first unit of it are fetched
    // while the current level is factored.
    int64_t first = level_unit_ptr[l0], end = level_unit_ptr[l0 + 1];
    Ilu0Unit cur = mine < end - first ? load_unit(units, first + mine) : NO_UNIT;
    for (int64_t l = l0; l < l1; ++l) {
        const int64_t count = end - first, next_end = l + 1 < l1 ? level_unit_ptr[l + 2] : end;
        const Ilu0Unit next = l + 1 < l1 && mine < next_end - end ? load_unit(units, end + mine) : NO_UNIT;
        factor_row(cur, rowptr, colidx, diag_pos, val, lu, lcol, lval);
        for (int64_t u0 = PASS; u0 < count; u0 += PASS) { // the same trip count in every thread
            const int64_t un = u0 + mine;
            factor_row(un < count ? load_unit(units, first + un) : NO_UNIT, rowptr, colidx, diag_pos, val, lu, lcol, lval);
        }
        __syncthreads(); // this level's rows of lu, stored by this workgroup, are what the next level loads
        first = end, end = next_end, cur = next;
    }
}

struct Launch {
    int64_t l0, l1; // levels
    bool chain;
};

struct Ilu0Plan {
    int dev = -1, flags = 0;
    int64_t n = 0, nnz = 0, levels = 0, wide = 0, chains = 0, widest = 0, longest = 0, long_rows = 0, chain_rows = 0;
    size_t bytes = 0;
    const int32_t *rowptr = nullptr, *colidx = nullptr; // the caller's
    DeviceBuffer buf;                                   // units | level_unit_ptr | diag_pos
    Ilu0Unit *units = nullptr;
    int64_t *level_unit_ptr = nullptr;
    int32_t *diag_pos = nullptr;
    std::vector<int64_t> h_level_unit_ptr;
    std::vector<Launch> launches;
};

inline size_t pad16(size_t b) { return (b + 15) / 16 * 16; }

} // namespace

extern "C" {

int sblas_hip_ilu0_plan_create(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx, int flags,
                               int64_t chain_rows, void **plan_out, int64_t *bad_row)
{
    if (bad_row) *bad_row = -1;
    if (!plan_out) return SBLAS_E_INVALID;
    *plan_out = nullptr;
    if (n < 0 || nnz < 0 || n > INT_MAX - 64 || nnz > INT_MAX || chain_rows < 0) return SBLAS_E_INVALID;
    if (flags != SBLAS_SPTRSV_AUTO && flags != SBLAS_SPTRSV_PER_LEVEL && flags != SBLAS_SPTRSV_CHAIN_ONLY) return SBLAS_E_INVALID;
    if ((n > 0 && !rowptr) || (nnz > 0 && !colidx)) return SBLAS_E_INVALID;
    std::unique_ptr<Ilu0Plan> p(new Ilu0Plan);
    p->dev = resolve_device(dev), p->flags = flags, p->n = n, p->nnz = nnz;
    p->rowptr = rowptr, p->colidx = colidx;
    p->chain_rows = chain_rows > 0 ? chain_rows : ILU0_CHAIN_ROWS;
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
    if (h_rowptr[n] != nnz) { // first, as in the solves: the host rule follows rowptr into a colidx of nnz entries
        if (bad_row) *bad_row = n - 1;
        return SBLAS_E_INVALID;
    }
    std::vector<int32_t> dpos((size_t)n), level((size_t)n);
    int rc = sblas_ilu0_check(n, h_rowptr.data(), h_colidx.data(), dpos.data(), bad_row);
    if (rc != SBLAS_OK) return rc;
    int64_t n_levels = 0;
    rc = sblas_sptrsv_levels(n, h_rowptr.data(), h_colidx.data(), SBLAS_FILL_LOWER, SBLAS_DIAG_NON_UNIT, level.data(), &n_levels, bad_row);
    if (rc != SBLAS_OK) return rc;
    p->levels = n_levels;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = (int64_t)h_rowptr[i + 1] - h_rowptr[i];
        p->longest = len > p->longest ? len : p->longest;
        p->long_rows += len > ILU0_LDS_MAX;
    }
    std::vector<Ilu0Unit> units;
    std::vector<int64_t> widths;
    ilu0_pack(n, h_rowptr.data(), dpos.data(), level.data(), n_levels, units, p->h_level_unit_ptr, widths);
    for (int64_t w : widths) p->widest = w > p->widest ? w : p->widest;

    // the launches
    std::vector<uint8_t> kind((size_t)n_levels);
    std::vector<int64_t> lfirst((size_t)n_levels + 1);
    int64_t n_launches = 0;
    if (sblas_sptrsv_schedule(n_levels, widths.data(), flags, p->chain_rows, kind.data(), lfirst.data(), &n_launches) != SBLAS_OK)
        return SBLAS_E_INVALID;
    for (int64_t q = 0; q < n_launches; ++q) {
        const bool chain = kind[q] == SBLAS_SPTRSV_LAUNCH_CHAIN;
        p->launches.push_back(Launch{lfirst[q], lfirst[q + 1], chain});
        ++(chain ? p->chains : p->wide);
    }

    const size_t o_up = units.size() * sizeof(Ilu0Unit), o_dpos = o_up + pad16(((size_t)n_levels + 1) * 8);
    const size_t total = o_dpos + pad16((size_t)n * 4);
    if (p->buf.alloc(p->dev, total) != hipSuccess) return SBLAS_E_HIP;
    p->bytes = total;
    p->units = p->buf.at<Ilu0Unit>(), p->level_unit_ptr = p->buf.at<int64_t>(o_up), p->diag_pos = p->buf.at<int32_t>(o_dpos);
    e = hipMemcpyAsync(p->units, units.data(), units.size() * sizeof(Ilu0Unit), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(p->level_unit_ptr, p->h_level_unit_ptr.data(), ((size_t)n_levels + 1) * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(p->diag_pos, dpos.data(), (size_t)n * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s); // the host vectors are read until here
    if (e != hipSuccess) return SBLAS_E_HIP;
    *plan_out = p.release();
    return SBLAS_OK;
}

int sblas_hip_ilu0_plan_info(const void *plan, int64_t out[12])
{
    if (!plan || !out) return SBLAS_E_INVALID;
    const Ilu0Plan *p = static_cast<const Ilu0Plan *>(plan);
    out[0] = p->n, out[1] = p->nnz, out[2] = p->levels, out[3] = (int64_t)p->launches.size(), out[4] = p->wide, out[5] = p->chains;
    out[6] = p->widest, out[7] = p->longest, out[8] = p->long_rows, out[9] = (int64_t)p->bytes, out[10] = p->flags, out[11] = p->chain_rows;
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
    if (!p) return SBLAS_E_INVALID;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    if (rowptr != p->rowptr || colidx != p->colidx) return SBLAS_E_INVALID;
    if (p->n == 0) return SBLAS_OK;
    if (!val || !lu) return SBLAS_E_INVALID; // n > 0: every row stores its diagonal
    hipStream_t s = (hipStream_t)stream;
    for (const Launch &q : p->launches) {
        if (q.chain) {
            ilu0_chain_kernel<<<1, ILU0_CHAIN_THREADS, 0, s>>>(q.l0, q.l1, p->level_unit_ptr, p->units, rowptr, colidx, p->diag_pos, val, lu);
        } else {
            const int64_t first = p->h_level_unit_ptr[q.l0], count = p->h_level_unit_ptr[q.l1] - first;
            const unsigned grid = (unsigned)((4 * count + ILU0_WIDE_THREADS - 1) / ILU0_WIDE_THREADS);
            ilu0_wide_kernel<<<grid, ILU0_WIDE_THREADS, 0, s>>>(first, count, p->units, rowptr, colidx, p->diag_pos, val, lu);
        }
    }
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

} // extern "C"
