// amg_aggregate.hip -- one level's aggregation of the AMG plan on the device: the pinned rule of
// amg_rule.cpp's amg_aggregate in Jones-Plassmann rounds, as color.hip runs the colouring.  Everything computed here is an
// integer or a comparison, so neither the lane width nor the schedule reaches a result: agg, aggptr, members and n_agg
// equal the host rule's, integer for integer.
//
// The rule in round form.  h(u) = color_priority(u, color_salt(seed + level)), computed from the index: there is no
// priority array.  Vertex v is decided by the strong neighbours u of its own row with h(u) > h(v) (the strength relation
// is not symmetric; only row v is consulted): a non-root as soon as one of them is a root, a root once all of them are
// non-roots, and otherwise it waits.  The greedy walk in descending h decides v from exactly those neighbours, and a
// state is final once written, so the rounds reach the walk's roots whatever the schedule.
//
// Lists.  A row of p stored entries belongs to G(p) lanes (the solves' 4 / 16 / 64, sptrsv_group_shift).  One kernel
// writes every row's width class, one stable radix pass on the class with the index as payload gives one ascending vertex
// list per width, and colptr_kernel on the sorted classes gives the three extents.  Every row kernel below is one launch
// per non-empty list; lane l walks the entries l, l + G, ... of its row.
//
// Bound (theta > 0 only).  bound[i] = theta * max_{k != i} |a_ik|, the product rounded once.  A lane's maximum is taken
// with the host's comparison `a > m` from m = 0, so a NaN entry is never a maximum; the lanes fold by a butterfly with
// the same comparison on values that are never NaN.  An infinite entry gives theta * inf, a row without off-diagonal
// entries 0.  An entry is strong when |a| >= bound, which a NaN never is.
//
// The round kernel.  A strong neighbour of higher h seen as a root makes v a non-root; one seen undecided makes v wait.
// The group votes by __ballot after every step and leaves at the first root seen.  state[v] goes from -1 to 0 or 1
// exactly once, by one aligned 4-byte store from the group's lane 0.
//
// Rounds are separate launches and nothing waits across workgroups: no cooperative launch, no polling.  state is read in
// place while other workgroups of the same launch write it, and that needs NO ordering between them:
//   - an entry changes once, from -1 to its final value, by one aligned 4-byte store: a load sees -1 or the final value;
//   - a neighbour seen decided (0 or 1) holds its final state, so a decision taken from it is the fixed point's;
//   - a neighbour seen as -1 (undecided, or decided in this launch and not yet visible) only makes v wait a round: no
//     decision is ever taken from an incomplete view;
//   - v becomes a root only after every strong neighbour of higher h was seen as 0, each of which is final.
// So a round decides at least what the synchronous form (sblas_amg_roots_rounds_ref) decides: the device needs at most
// that many rounds, and how many it takes is not part of the contract.  The kernel boundary is the only release the next
// round relies on.  state is not __restrict__ and is never read through a wave-uniform address, which keeps it on the
// vector path.
//
// Termination.  One atomicAdd per wave that decided any vertex, onto that round's counter.  The host launches batches of
// rounds (4, 8, ... up to 32), reads the batch's counters and stops when the sum reaches n; rounds launched past that
// point find nothing to do.  The undecided vertex of greatest h waits for nobody, so a round that decides nothing while
// vertices remain is a bug: SBLAS_E_INTERNAL instead of spinning.
//
// Join: a separate pass after the last round.  v's aggregate is the first root among ALL its strong neighbours in stored
// order, and a neighbour of lower h that became a root later can precede the one that made v a non-root, so the join
// cannot ride in the rounds.  The roots are numbered by an exclusive scan of the root flags (radix_sort.h's scan): the
// ascending vertex order, and the total is n_agg.  Then one launch per list: the earliest step with a strong root
// neighbour, and within it the lowest lane (__ffsll of the group's ballot), writes agg[v] = number[u].
//
// Members: the vertices by (aggregate, vertex): radix_sort.h's stable passes on agg with the index as payload, as many
// 8-bit passes as n_agg needs; aggptr is colptr_kernel on the sorted keys.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include "../../include/sblas_hip.h"
#include "amg.h"
#include "capi_util.h"
#include "color.h"
#include "radix_sort.h"

using namespace sblas;

namespace {

constexpr int ROUND_BATCH_MAX = 32; // rounds launched between two reads of the counters
constexpr int WIDTHS = 3;           // 4, 16 and 64 lanes

struct Layout {
    size_t bound = 0, state = 0, number = 0, list = 0, klass = 0, words = 0, nbsum = 0, sort = 0, total = 0;
    int64_t number_blocks = 0;
};

// bound (n doubles) | state (n) | number (n + 1) | list (n) | class (n) | counters (32) and the list extents (4) | the
// scan's block sums | the sort's workspace
Layout layout_of(int64_t n)
{
    Layout L;
    const size_t arr = align16((size_t)n * 4);
    size_t off = 0;
    L.bound = off, off += align16((size_t)n * 8);
    L.state = off, off += arr;
    L.number = off, off += align16(((size_t)n + 1) * 4);
    L.list = off, off += arr;
    L.klass = off, off += arr;
    L.words = off, off += align16((ROUND_BATCH_MAX + WIDTHS + 1) * 4);
    L.number_blocks = ceil_div(n + 1, SCAN_TILE);
    L.nbsum = off, off += align16((size_t)L.number_blocks * 4);
    L.sort = off, off += workspace_layout(n, nullptr, nullptr);
    L.total = off;
    return L;
}

// the lanes of this thread's group of G = 1 << SHIFT, as a ballot mask
template <int SHIFT> __device__ __forceinline__ uint64_t group_mask(int lane)
{
    constexpr int G = 1 << SHIFT;
    return (G == 64 ? ~0ull : ((1ull << G) - 1ull)) << (lane - (lane & (G - 1)));
}

__global__ __launch_bounds__(AMG_THREADS) void agg_class_kernel(int64_t n, const int32_t *__restrict__ rowptr, int32_t *__restrict__ klass)
{
    const int64_t i = (int64_t)blockIdx.x * AMG_THREADS + threadIdx.x;
    if (i < n) klass[i] = (sptrsv_group_shift((int64_t)rowptr[i + 1] - rowptr[i]) - 2) / 2;
}

__global__ __launch_bounds__(AMG_THREADS) void agg_iota_kernel(int64_t n, int32_t *__restrict__ a)
{
    const int64_t i = (int64_t)blockIdx.x * AMG_THREADS + threadIdx.x;
    if (i < n) a[i] = (int32_t)i;
}

// bound[v] for the vertices list[0 .. count - 1]
template <int SHIFT>
__global__ __launch_bounds__(AMG_THREADS) void agg_bound_kernel(int64_t count, const int32_t *__restrict__ list, const int32_t *__restrict__ rowptr,
                                                                const int32_t *__restrict__ colidx, const double *__restrict__ val, double theta,
                                                                double *__restrict__ bound)
{
    constexpr int G = 1 << SHIFT;
    const int ln = (int)threadIdx.x & (G - 1);
    const int64_t slot = ((int64_t)blockIdx.x * AMG_THREADS + threadIdx.x) >> SHIFT;
    const int32_t v = slot < count ? list[slot] : -1; // whole groups: the butterfly stays inside one
    double m = 0.0;
    if (v >= 0) {
        const int64_t a0 = rowptr[v], a1 = rowptr[v + 1];
        for (int64_t e = a0 + ln; e < a1; e += G) {
            const double a = fabs(val[e]);
            if (colidx[e] != v && a > m) m = a; // the host's comparison: a NaN is never taken
        }
    }
#pragma unroll
    for (int o = 1; o < G; o <<= 1) {
        const double y = __shfl_xor(m, o, 64);
        if (y > m) m = y;
    }
    if (v >= 0 && ln == 0) bound[v] = theta * m;
}

// One round over the vertices list[0 .. count - 1], which all have G = 1 << SHIFT lanes.  state: see the header comment.
template <int SHIFT>
__global__ __launch_bounds__(AMG_THREADS) void agg_round_kernel(int64_t count, const int32_t *__restrict__ list, const int32_t *__restrict__ rowptr,
                                                                const int32_t *__restrict__ colidx, const double *__restrict__ val,
                                                                const double *__restrict__ bound, uint32_t salt, int32_t *state,
                                                                uint32_t *__restrict__ decided)
{
    constexpr int G = 1 << SHIFT;
    const int lane = (int)threadIdx.x & 63, ln = lane & (G - 1);
    const uint64_t group = group_mask<SHIFT>(lane);
    const int64_t slot = ((int64_t)blockIdx.x * AMG_THREADS + threadIdx.x) >> SHIFT;
    bool took = false;
    const int32_t v = slot < count ? list[slot] : -1; // whole groups: nothing below crosses a group
    if (v >= 0 && state[v] < 0) {
        const int64_t a0 = rowptr[v];
        const int p = (int)(rowptr[v + 1] - a0);
        const uint32_t hv = color_priority((uint32_t)v, salt);
        const double bv = val ? bound[v] : 0.0;
        bool non_root = false, wait = false;
        for (int e0 = 0; e0 < p; e0 += G) { // the same trip count in every lane of the group
            const int e = e0 + ln;
            bool is_root = false, open = false;
            if (e < p) {
                const int32_t u = colidx[a0 + e];
                if (u != v && (!val || fabs(val[a0 + e]) >= bv) && color_priority((uint32_t)u, salt) > hv) {
                    const int32_t su = state[u];
                    is_root = su == 1, open = su < 0;
                }
            }
            if ((__ballot(is_root) & group) != 0) { // the vote: the first root seen ends the walk
                non_root = true;
                break;
            }
            wait = wait || (__ballot(open) & group) != 0;
        }
        if (non_root || !wait) {
            if (ln == 0) state[v] = non_root ? 0 : 1;
            took = ln == 0;
        }
    }
    const uint64_t m = __ballot(took);
    if (lane == 0 && m != 0) atomicAdd(decided, (uint32_t)__popcll(m));
}

// number[v] = 1 for a root, 0 otherwise, and number[n] = 0: the scan's input
__global__ __launch_bounds__(AMG_THREADS) void agg_flag_kernel(int64_t n, const int32_t *__restrict__ state, uint32_t *__restrict__ number)
{
    const int64_t i = (int64_t)blockIdx.x * AMG_THREADS + threadIdx.x;
    if (i <= n) number[i] = i < n && state[i] == 1 ? 1u : 0u;
}

// agg[v]: a root's own number, otherwise the number of the first root among v's strong neighbours in stored order
template <int SHIFT>
__global__ __launch_bounds__(AMG_THREADS) void agg_join_kernel(int64_t count, const int32_t *__restrict__ list, const int32_t *__restrict__ rowptr,
                                                               const int32_t *__restrict__ colidx, const double *__restrict__ val,
                                                               const double *__restrict__ bound, const int32_t *__restrict__ state,
                                                               const uint32_t *__restrict__ number, int32_t *__restrict__ agg)
{
    constexpr int G = 1 << SHIFT;
    const int lane = (int)threadIdx.x & 63, ln = lane & (G - 1);
    const uint64_t group = group_mask<SHIFT>(lane);
    const int64_t slot = ((int64_t)blockIdx.x * AMG_THREADS + threadIdx.x) >> SHIFT;
    const int32_t v = slot < count ? list[slot] : -1;
    if (v < 0) return; // whole groups
    if (state[v] == 1) {
        if (ln == 0) agg[v] = (int32_t)number[v];
        return;
    }
    const int64_t a0 = rowptr[v];
    const int p = (int)(rowptr[v + 1] - a0);
    const double bv = val ? bound[v] : 0.0;
    for (int e0 = 0; e0 < p; e0 += G) {
        const int e = e0 + ln;
        int32_t u = -1;
        if (e < p) {
            const int32_t c = colidx[a0 + e];
            if (c != v && (!val || fabs(val[a0 + e]) >= bv) && state[c] == 1) u = c;
        }
        const uint64_t b = __ballot(u >= 0) & group;
        if (b != 0) { // the earliest step, and within it the lowest lane: the first in stored order
            if (lane == __ffsll((unsigned long long)b) - 1) agg[v] = (int32_t)number[u];
            return;
        }
    }
}

template <typename F> void per_list(const int64_t *ext, F launch)
{
    for (int t = 0; t < WIDTHS; ++t) {
        const int64_t count = ext[t + 1] - ext[t];
        if (count == 0) continue;
        const int shift = 2 + 2 * t;
        launch(t, ext[t], count, (unsigned)(((count << shift) + AMG_THREADS - 1) / AMG_THREADS));
    }
}

inline unsigned grid_of(int64_t threads) { return (unsigned)((threads + AMG_THREADS - 1) / AMG_THREADS); }

} // namespace

extern "C" {

size_t sblas_hip_amg_aggregate_workspace(int64_t n, int64_t nnz)
{
    (void)&gather_f64_kernel; // radix_sort.h's gather is not used here
    if (n <= 0 || nnz < 0 || n > INT_MAX || nnz > INT_MAX) return 0;
    return layout_of(n).total;
}

int sblas_hip_amg_aggregate_i32(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx, const double *val,
                                double theta, uint32_t seed, uint32_t level, int32_t *agg, int32_t *aggptr, int32_t *members, void *workspace,
                                size_t workspace_bytes, int64_t *n_agg, int64_t *rounds)
{
    if (n_agg) *n_agg = 0;
    if (rounds) *rounds = 0;
    if (n < 0 || nnz < 0 || n > INT_MAX || nnz > INT_MAX || (n == 0 && nnz != 0) || !n_agg || !rounds || !aggptr) return SBLAS_E_INVALID;
    if (!amg_theta_ok(theta) || (theta > 0.0 && !val)) return SBLAS_E_INVALID;
    if (n > 0 && (!rowptr || !agg || !members || (nnz > 0 && !colidx))) return SBLAS_E_INVALID;
    const size_t need = sblas_hip_amg_aggregate_workspace(n, nnz);
    if (need > 0 && (!workspace || workspace_bytes < need)) return SBLAS_E_WORKSPACE;
    if (!aligned16(workspace)) return SBLAS_E_INVALID;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        if (hipMemsetAsync(aggptr, 0, 4, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return SBLAS_E_HIP;
        return SBLAS_OK;
    }
    const bool by_value = theta > 0.0;
    const double *sval = by_value ? val : nullptr; // structure only: every off-diagonal entry is strong
    const Layout L = layout_of(n);
    char *base = static_cast<char *>(workspace);
    double *bound = reinterpret_cast<double *>(base + L.bound);
    int32_t *state = reinterpret_cast<int32_t *>(base + L.state), *list = reinterpret_cast<int32_t *>(base + L.list);
    int32_t *klass = reinterpret_cast<int32_t *>(base + L.klass);
    uint32_t *number = reinterpret_cast<uint32_t *>(base + L.number), *counters = reinterpret_cast<uint32_t *>(base + L.words);
    int32_t *d_ext = reinterpret_cast<int32_t *>(base + L.words) + ROUND_BATCH_MAX;
    uint32_t *nbsum = reinterpret_cast<uint32_t *>(base + L.nbsum);
    Workspace w;
    workspace_layout(n, base + L.sort, &w);

    // the lists: the vertices by (width class, vertex), and where each class begins
    agg_class_kernel<<<grid_of(n), AMG_THREADS, 0, s>>>(n, rowptr, klass);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = radix_pass(s, w, klass, nullptr, n, 0, 0);
    if (e == hipSuccess) e = hipMemcpyAsync(list, w.idx[0], (size_t)n * 4, hipMemcpyDeviceToDevice, s);
    int32_t h_ext[WIDTHS + 1] = {0, 0, 0, 0};
    if (e == hipSuccess) {
        colptr_kernel<<<1, T_THREADS, 0, s>>>(w.keys[0], n, WIDTHS, nullptr, d_ext);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemsetAsync(state, 0xff, (size_t)n * 4, s); // every vertex -1
    if (e == hipSuccess) e = hipMemcpyAsync(h_ext, d_ext, sizeof(h_ext), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return SBLAS_E_HIP;
    int64_t ext[WIDTHS + 1];
    for (int t = 0; t <= WIDTHS; ++t) ext[t] = h_ext[t];
    if (ext[0] != 0 || ext[WIDTHS] != n || ext[1] < 0 || ext[1] > ext[2] || ext[2] > n) return SBLAS_E_INTERNAL;

    if (by_value) {
        per_list(ext, [&](int t, int64_t first, int64_t count, unsigned grid) {
            if (t == 0) agg_bound_kernel<2><<<grid, AMG_THREADS, 0, s>>>(count, list + first, rowptr, colidx, sval, theta, bound);
            else if (t == 1) agg_bound_kernel<4><<<grid, AMG_THREADS, 0, s>>>(count, list + first, rowptr, colidx, sval, theta, bound);
            else agg_bound_kernel<6><<<grid, AMG_THREADS, 0, s>>>(count, list + first, rowptr, colidx, sval, theta, bound);
        });
        if (hipGetLastError() != hipSuccess) return SBLAS_E_HIP;
    }

    const uint32_t salt = color_salt(seed + level);
    int64_t left = n, done = 0;
    for (int batch = 4; left > 0; batch = batch * 2 < ROUND_BATCH_MAX ? batch * 2 : ROUND_BATCH_MAX) {
        e = hipMemsetAsync(counters, 0, ROUND_BATCH_MAX * sizeof(uint32_t), s);
        for (int r = 0; r < batch && e == hipSuccess; ++r) {
            per_list(ext, [&](int t, int64_t first, int64_t count, unsigned grid) {
                if (t == 0) agg_round_kernel<2><<<grid, AMG_THREADS, 0, s>>>(count, list + first, rowptr, colidx, sval, bound, salt, state, counters + r);
                else if (t == 1) agg_round_kernel<4><<<grid, AMG_THREADS, 0, s>>>(count, list + first, rowptr, colidx, sval, bound, salt, state, counters + r);
                else agg_round_kernel<6><<<grid, AMG_THREADS, 0, s>>>(count, list + first, rowptr, colidx, sval, bound, salt, state, counters + r);
            });
            e = hipGetLastError();
        }
        uint32_t h_counters[ROUND_BATCH_MAX];
        if (e == hipSuccess) e = hipMemcpyAsync(h_counters, counters, (size_t)batch * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return SBLAS_E_HIP;
        for (int r = 0; r < batch && left > 0; ++r) {
            if (h_counters[r] == 0 || (int64_t)h_counters[r] > left) return SBLAS_E_INTERNAL; // no progress: never spin
            left -= h_counters[r];
            ++done;
        }
    }

    // the join: the roots numbered in ascending vertex order, then every vertex's aggregate
    agg_flag_kernel<<<grid_of(n + 1), AMG_THREADS, 0, s>>>(n, state, number);
    e = hipGetLastError();
    if (e == hipSuccess) e = scan_exclusive(s, number, n + 1, nbsum, L.number_blocks);
    if (e != hipSuccess) return SBLAS_E_HIP;
    per_list(ext, [&](int t, int64_t first, int64_t count, unsigned grid) {
        if (t == 0) agg_join_kernel<2><<<grid, AMG_THREADS, 0, s>>>(count, list + first, rowptr, colidx, sval, bound, state, number, agg);
        else if (t == 1) agg_join_kernel<4><<<grid, AMG_THREADS, 0, s>>>(count, list + first, rowptr, colidx, sval, bound, state, number, agg);
        else agg_join_kernel<6><<<grid, AMG_THREADS, 0, s>>>(count, list + first, rowptr, colidx, sval, bound, state, number, agg);
    });
    uint32_t total = 0;
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&total, number + n, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return SBLAS_E_HIP;
    if (total == 0 || (int64_t)total > n) return SBLAS_E_INTERNAL; // the vertex of greatest h is a root

    // members: the vertices by (aggregate, vertex); aggptr from the sorted keys
    const int32_t *skeys = agg, *sidx = nullptr;
    const int passes = radix_passes((int64_t)total);
    for (int q = 0; q < passes; ++q) {
        if (radix_pass(s, w, skeys, sidx, n, q * RADIX_BITS, q & 1) != hipSuccess) return SBLAS_E_HIP;
        skeys = w.keys[q & 1], sidx = w.idx[q & 1];
    }
    if (sidx) e = hipMemcpyAsync(members, sidx, (size_t)n * 4, hipMemcpyDeviceToDevice, s);
    else agg_iota_kernel<<<grid_of(n), AMG_THREADS, 0, s>>>(n, members); // one aggregate: already in order
    colptr_kernel<<<grid_for((int64_t)total + 1), T_THREADS, 0, s>>>(skeys, n, (int64_t)total, nullptr, aggptr);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return SBLAS_E_HIP;
    *n_agg = (int64_t)total, *rounds = done;
    return SBLAS_OK;
}

} // extern "C"
