// level_kernels.h -- the HIP side of a level plan, shared by sptrsv.hip and ilu0.hip: what the two plans hold in common
// with the checks around it, and the two walks over a level's units that their kernels instantiate.
//
// A solve or a factorisation is a fixed sequence of launches of two kernels:
//   wide   one level a launch; the level's rows, in ascending row order, spread over the grid;
//   chain  one workgroup walks a run of consecutive levels with __syncthreads() between them.
// Nothing waits across workgroups: no flag polling, no cooperative launch, no grid barrier, no atomics.  The only
// synchronisation is the kernel boundary and __syncthreads(), and every loop's trip count comes from the plan.
//
// Visibility inside a chain launch.  The array the rows produce (x, lu) is written with plain global stores and read
// with plain global loads.  __syncthreads() is a workgroup-scope release and acquire around the barrier: every wave
// waits for its stores (s_waitcnt vmcnt(0)) before it arrives, and no load of that array for a later level is issued
// before it leaves (what is fetched ahead of the barrier is plan data, which no kernel writes).  The waves of one
// workgroup run on one CU and share its vector L1, which is write-through and sees the CU's own stores; the hazard of a
// stale L1 line exists only between CUs, and no other workgroup runs in a chain launch.  Between launches the kernel
// boundary orders everything.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "capi_util.h"
#include "level_plan.h"

namespace {

// one 16-byte load of a record of four int32
template <typename U> __device__ __forceinline__ U load_unit(const U *__restrict__ units, int64_t u)
{
    static_assert(sizeof(U) == 16, "one 16-byte load per unit");
    const int4 v = *reinterpret_cast<const int4 *>(units + u);
    return U{v.x, v.y, v.z, v.w};
}

// wide: this thread's unit among the level's units first .. first + count - 1, four lanes each
template <int THREADS, typename U>
__device__ __forceinline__ U wide_unit(int64_t first, int64_t count, const U *__restrict__ units, const U pad)
{
    const int64_t u = ((int64_t)blockIdx.x * THREADS + threadIdx.x) >> 2;
    return u < count ? load_unit(units, first + u) : pad;
}
inline unsigned wide_grid(int64_t lanes, int threads) { return (unsigned)((lanes + threads - 1) / threads); }

// chain: levels l0 .. l1 - 1 in one workgroup of THREADS threads, row(unit) for each of this thread's units; a level wider
// than the workgroup is looped over.  The plan's arrays do not depend on what the rows produce: the next level's extent
// and this thread's first unit of it are fetched while the current level runs, so that behind the barrier only the
// row's own data is waited for.
template <int THREADS, typename U, typename F>
__device__ __forceinline__ void chain_walk(int64_t l0, int64_t l1, const int64_t *__restrict__ level_unit_ptr,
                                           const U *__restrict__ units, const U pad, F row)
{
    constexpr int PASS = THREADS / 4; // units of one pass
    const int mine = threadIdx.x >> 2;
    int64_t first = level_unit_ptr[l0], end = level_unit_ptr[l0 + 1];
    U cur = mine < end - first ? load_unit(units, first + mine) : pad;
    for (int64_t l = l0; l < l1; ++l) {
        const int64_t count = end - first, next_end = l + 1 < l1 ? level_unit_ptr[l + 2] : end;
        const U next = l + 1 < l1 && mine < next_end - end ? load_unit(units, end + mine) : pad;
        row(cur);
        for (int64_t u0 = PASS; u0 < count; u0 += PASS) { // the same trip count in every thread
            const int64_t u = u0 + mine;
            row(u < count ? load_unit(units, first + u) : pad);
        }
        __syncthreads(); // this level's rows, stored by this workgroup, are what the next level loads
        first = end, end = next_end, cur = next;
    }
}

// what the two plans hold in common
struct LevelPlan {
    int dev = -1, flags = 0;
    int64_t n = 0, nnz = 0, levels = 0, longest = 0, chain_rows = 0;
    size_t bytes = 0;
    const int32_t *rowptr = nullptr, *colidx = nullptr; // the caller's
    DeviceBuffer buf;
    int64_t *level_unit_ptr = nullptr;
    std::vector<int64_t> h_level_unit_ptr;
    sblas::LaunchList sched;
};

// the head of a create: the outputs cleared, the arguments the two creates share checked (false: refuse) and kept in p
inline bool level_plan_begin(LevelPlan &p, int dev, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx, int flags,
                             int64_t chain_rows, int64_t default_chain_rows, void **plan_out, int64_t *bad_row)
{
    if (bad_row) *bad_row = -1;
    if (!plan_out) return false;
    *plan_out = nullptr;
    if (n < 0 || nnz < 0 || n > INT_MAX - 64 || nnz > INT_MAX || chain_rows < 0 || (n == 0 && nnz != 0)) return false;
    if (flags != SBLAS_SPTRSV_AUTO && flags != SBLAS_SPTRSV_PER_LEVEL && flags != SBLAS_SPTRSV_CHAIN_ONLY) return false;
    p.dev = resolve_device(dev), p.flags = flags, p.n = n, p.nnz = nnz, p.rowptr = rowptr, p.colidx = colidx;
    p.chain_rows = chain_rows > 0 ? chain_rows : default_chain_rows;
    return (n == 0 || rowptr) && (nnz == 0 || colidx);
}

// SBLAS_OK when the plan lives on device `dev` (< 0: the current one) and was made for exactly this structure: the check
// before every planned call
inline int level_plan_speaks_for(const LevelPlan *p, int dev, const int32_t *rowptr, const int32_t *colidx)
{
    if (!p || p->dev != resolve_device(dev)) return SBLAS_E_INVALID;
    return rowptr == p->rowptr && colidx == p->colidx ? SBLAS_OK : SBLAS_E_INVALID;
}

} // namespace
