// color.hip -- the multicolour ordering on the device: a graph colouring of a square CSR pattern
// (sblas_hip_color_plan_*) and the symmetric permutation B = P A P^T of a CSR matrix on a plan (sblas_hip_permute_plan_*).
//
// Colouring.  u is a neighbour of v when u != v and the pattern stores (v, u) or (u, v).  color[v] is what the scalar
// loop of color_rule.cpp gives: first fit in descending h(v) = fmix32(v + salt).  The device runs the Jones-Plassmann
// form of it in rounds, one launch each: an uncoloured vertex none of whose uncoloured neighbours has a higher h takes
// the smallest colour no coloured neighbour holds.  A vertex's colour is a function of the colours of its neighbours of
// higher h alone, and it is not coloured before all of them are, so the colours do not depend on the schedule.
//
// The round kernel.  A vertex of p = len(row v of A) + len(row v of A^T) stored entries belongs to G(p) lanes (the
// solves' 4 / 16 / 64); the plan keeps one ascending vertex list per width and a round is one launch per non-empty list.
// Lane l walks the entries l, l + G, ... of the two rows, one after the other as one sequence.
//   pass 0    decides eligibility and gathers the colours below COLOR_WINDOW: a neighbour with color < 0 and a higher h is
//             a hit, and the group votes after every step and leaves at the first one; a coloured neighbour sets its bit
//             in the lane's 64-bit mask.  The masks are OR-folded by a butterfly and the first clear bit is the colour.
//   pass w    when the window is full, the walk is repeated for the colours [w * 64, w * 64 + 64).  First fit is at most
//             the number of distinct neighbours, so the passes end at w * 64 <= p.
// h is computed from the index: there is no priority array.
//
// Rounds are separate launches and nothing waits across workgroups.  color is read in place while other groups of the
// same launch write it.  That is sound without any ordering between them: an entry changes once, from -1 to its final
// value, by one aligned 4-byte store, and
//   - a neighbour of lower h is never coloured before v is (it would need v coloured), so whatever copy of its entry a
//     lane sees is -1, in every pass;
//   - a neighbour of higher h seen as -1 (not yet coloured, or coloured in this launch and not yet visible) is a hit: v
//     waits a round, and no colour is taken from an incomplete view;
//   - a neighbour of higher h seen coloured holds its final colour.
// So the device needs at most the host rule's sync_rounds rounds, and how many it takes is not part of the contract.
// color is not __restrict__ and is never read through a uniform address, which keeps it off the scalar path.
//
// Termination.  A round's launches add the vertices they coloured to that round's counter (one atomic per wave that
// coloured any).  The host launches a batch of rounds, reads the batch's counters and stops when the sum reaches n;
// rounds launched past that point find nothing to do.  The uncoloured vertex of greatest h is always eligible, so a
// round that colours nothing while vertices remain is a bug: create returns SBLAS_E_INTERNAL instead of spinning.
//
// Order.  perm = the vertices by (colour, v): radix_sort.h's stable passes on the colours with the index as payload, as
// many 8-bit passes as the bound 1 + (the greatest p) on the colours needs; inv is scattered from perm and color_ptr is
// colptr_kernel on the sorted colours.
//
// Permutation.  Row r of B holds the entries of row perm[r] of A with columns inv[col], ascending by new column, equal
// columns in A's stored order.  A relabel kernel writes the triplets (inv[row(e)], inv[col(e)]) and the COO plan
// (SBLAS_COO_KEEP) sorts them stably by (row, col): its rowptr, colidx and entry permutation are B's rowptr, colidx and
// src.  values() is one gather through src: one launch, no allocation.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <memory>
#include <vector>
#include "../../include/sblas_hip.h"
#include "capi_util.h"
#include "color.h"
#include "radix_sort.h"

using namespace sblas;

namespace {

constexpr int ROUND_BATCH_MAX = 32; // rounds launched between two reads of the counters

// One round over the vertices list[0 .. count - 1], which all have G = 1 << SHIFT lanes.  color: see the header comment.
template <int SHIFT>
__global__ __launch_bounds__(COLOR_THREADS) void color_round_kernel(int64_t count, const int32_t *__restrict__ list,
                                                                    const int32_t *__restrict__ rowptr,
                                                                    const int32_t *__restrict__ colidx,
                                                                    const int32_t *__restrict__ tptr,
                                                                    const int32_t *__restrict__ tidx, uint32_t salt, int32_t *color,
                                                                    uint32_t *__restrict__ coloured)
{
    constexpr int G = 1 << SHIFT;
    const int lane = (int)threadIdx.x & 63, ln = lane & (G - 1);
    // the lanes of this group, as a ballot mask
    const uint64_t group = (G == 64 ? ~0ull : ((1ull << G) - 1ull)) << (lane - ln);
    const int64_t slot = ((int64_t)blockIdx.x * COLOR_THREADS + threadIdx.x) >> SHIFT;
    bool took = false;
    const int32_t v = slot < count ? list[slot] : -1; // whole groups: nothing below crosses a group
    if (v >= 0 && color[v] < 0) {
        const int64_t a0 = rowptr[v], t0 = tptr[v];
        const int la = (int)(rowptr[v + 1] - a0), p = la + (int)(tptr[v + 1] - t0);
        const uint32_t hv = color_priority((uint32_t)v, salt);
        int32_t c = -1;
        bool wait = false;
        for (int w = 0; w == 0 || (int64_t)w * COLOR_WINDOW <= p; ++w) { // the same trip counts in every lane of the group
            const int32_t base = w * COLOR_WINDOW;
            uint64_t mask = 0;
            for (int e0 = 0; e0 < p; e0 += G) {
                const int e = e0 + ln;
                bool hit = false;
                if (e < p) {
                    const int32_t u = e < la ? colidx[a0 + e] : tidx[t0 + (e - la)];
                    if (u != v) {
                        const int32_t cu = color[u];
                        if (cu < 0) hit = w == 0 && color_priority((uint32_t)u, salt) > hv;
                        else if (cu >= base && cu < base + COLOR_WINDOW) mask |= 1ull << (cu - base);
                    }
                }
                if (w == 0 && (__ballot(hit) & group) != 0) { // the vote: the first hit ends the walk
                    wait = true;
                    break;
                }
            }
            if (wait) break;
#pragma unroll
            for (int o = 1; o < G; o <<= 1) mask |= __shfl_xor(mask, o, 64); // partners stay inside the group
            if (mask != ~0ull) {
                c = base + (__ffsll((unsigned long long)~mask) - 1);
                break;
            }
        }
        if (c >= 0) {
            if (ln == 0) color[v] = c;
            took = ln == 0;
        }
    }
    const uint64_t m = __ballot(took);
    if (lane == 0 && m != 0) atomicAdd(coloured, (uint32_t)__popcll(m));
}

// perm[i] = the i-th vertex by (colour, vertex) (sidx == nullptr: the identity) and inv[perm[i]] = i
__global__ __launch_bounds__(T_THREADS) void color_order_kernel(const int32_t *__restrict__ sidx, int64_t n, int32_t *__restrict__ perm,
                                                                int32_t *__restrict__ inv)
{
    for (int64_t i = (int64_t)blockIdx.x * T_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * T_THREADS) {
        const int32_t v = sidx ? sidx[i] : (int32_t)i;
        perm[i] = v;
        inv[v] = (int32_t)i;
    }
}

struct ColorPlan {
    int dev = -1;
    int64_t n = 0, nnz = 0, colors = 0, rounds = 0, largest = 0, smallest = 0, degree = 0;
    size_t bytes = 0;
    DeviceBuffer buf; // color | perm | inv | color_ptr
    int32_t *color = nullptr, *perm = nullptr, *inv = nullptr, *color_ptr = nullptr;
};

__global__ __launch_bounds__(T_THREADS) void permute_fill_kernel(int64_t n, int32_t value, int32_t *__restrict__ a)
{
    for (int64_t i = (int64_t)blockIdx.x * T_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * T_THREADS) a[i] = value;
}

// first[q] = the least i with perm[i] == q (INT_MAX: none); an entry outside [0, n) lowers *bad to its index
__global__ __launch_bounds__(T_THREADS) void permute_first_kernel(int64_t n, const int32_t *__restrict__ perm, int32_t *first, int32_t *bad)
{
    for (int64_t i = (int64_t)blockIdx.x * T_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * T_THREADS) {
        const int32_t q = perm[i];
        if (q < 0 || (int64_t)q >= n) atomicMin(bad, (int32_t)i);
        else atomicMin(first + q, (int32_t)i);
    }
}

// a repeated entry: its second and later places are not the first; where perm is a permutation, first is its inverse
__global__ __launch_bounds__(T_THREADS) void permute_repeat_kernel(int64_t n, const int32_t *__restrict__ perm,
                                                                   const int32_t *__restrict__ first, int32_t *bad)
{
    for (int64_t i = (int64_t)blockIdx.x * T_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * T_THREADS) {
        const int32_t q = perm[i];
        if (q >= 0 && (int64_t)q < n && first[q] != (int32_t)i) atomicMin(bad, (int32_t)i);
    }
}

// entry e of A, in row r (rowptr[r] <= e < rowptr[r + 1]), is the triplet (inv[r], inv[col(e)]) of B
__global__ __launch_bounds__(T_THREADS) void permute_relabel_kernel(int64_t nnz, int64_t n, const int32_t *__restrict__ rowptr,
                                                                    const int32_t *__restrict__ colidx, const int32_t *__restrict__ inv,
                                                                    int32_t *__restrict__ trow, int32_t *__restrict__ tcol)
{
    for (int64_t e = (int64_t)blockIdx.x * T_THREADS + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * T_THREADS) {
        int64_t lo = 0, hi = n - 1; // the last row whose start is <= e (empty rows share their start with the next)
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (rowptr[mid] <= e) lo = mid;
            else hi = mid - 1;
        }
        trow[e] = inv[lo];
        tcol[e] = inv[colidx[e]];
    }
}

struct PermutePlan {
    int dev = -1;
    int64_t n = 0, nnz = 0;
    size_t bytes = 0;
    DeviceBuffer buf; // inv
    int32_t *inv = nullptr;
    void *coo = nullptr; // B's rowptr, colidx and src
    const int32_t *src = nullptr;
    ~PermutePlan() { sblas_hip_coo_plan_destroy(coo); }
};

} // namespace

extern "C" {

int sblas_hip_color_plan_create(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                                uint32_t seed, void **plan_out, int64_t *bad_row)
{
    if (bad_row) *bad_row = -1;
    if (!plan_out) return SBLAS_E_INVALID;
    *plan_out = nullptr;
    if (n < 0 || nnz < 0 || n > INT_MAX - 64 || nnz > INT_MAX) return SBLAS_E_INVALID;
    if ((n > 0 && !rowptr) || (nnz > 0 && !colidx)) return SBLAS_E_INVALID;
    std::unique_ptr<ColorPlan> p(new ColorPlan);
    p->dev = resolve_device(dev), p->n = n, p->nnz = nnz;
    if (n == 0) {
        if (nnz != 0) return SBLAS_E_INVALID;
        *plan_out = p.release();
        return SBLAS_OK;
    }
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    hipStream_t s = (hipStream_t)stream;

    // the structure comes to the host once, as in the solves: the check, and which lane group takes each vertex
    std::vector<int32_t> h_rowptr, h_colidx;
    const int frc = fetch_structure(s, n, nnz, rowptr, colidx, h_rowptr, h_colidx, bad_row);
    if (frc != SBLAS_OK) return frc;
    hipError_t e = hipSuccess;
    std::vector<int32_t> lists[3]; // the vertices of 4, 16 and 64 lanes, ascending
    {
        std::vector<int32_t> h_tptr, h_tidx;
        const int rc = color_check_transpose(n, h_rowptr.data(), h_colidx.data(), h_tptr, h_tidx, bad_row);
        if (rc != SBLAS_OK) return rc;
        for (int64_t v = 0; v < n; ++v) {
            const int64_t deg = ((int64_t)h_rowptr[v + 1] - h_rowptr[v]) + ((int64_t)h_tptr[v + 1] - h_tptr[v]);
            if (deg > INT_MAX) return SBLAS_E_INVALID; // the kernel counts a vertex's entries in an int
            p->degree = deg > p->degree ? deg : p->degree;
            lists[(sptrsv_group_shift(deg) - 2) / 2].push_back((int32_t)v);
        }
    }
    // a colour is at most the number of distinct neighbours: the sort's key range, known before any colour is
    const int64_t color_bound = p->degree + 1 < n ? p->degree + 1 : n;

    const size_t arr = align16((size_t)n * 4), cp = align16(((size_t)color_bound + 1) * 4);
    p->bytes = 3 * arr + cp;
    if (p->buf.alloc(p->dev, p->bytes) != hipSuccess) return SBLAS_E_HIP;
    p->color = p->buf.at<int32_t>(), p->perm = p->buf.at<int32_t>(arr), p->inv = p->buf.at<int32_t>(2 * arr);
    p->color_ptr = p->buf.at<int32_t>(3 * arr);

    // create's own scratch, freed before it returns: A^T | the vertex lists | the round counters | the workspace
    const size_t tp = align16(((size_t)n + 1) * 4), ti = align16((size_t)nnz * 4), cn = align16(ROUND_BATCH_MAX * sizeof(uint32_t));
    const size_t tws = sblas_hip_csr_transpose_workspace(n, n, nnz), sws = workspace_layout(n, nullptr, nullptr);
    const size_t wsb = tws > sws ? tws : sws;
    DeviceBuffer scratch;
    if (scratch.alloc(p->dev, tp + ti + arr + cn + wsb) != hipSuccess) return SBLAS_E_HIP;
    int32_t *tptr = scratch.at<int32_t>(), *tidx = scratch.at<int32_t>(tp), *list = scratch.at<int32_t>(tp + ti);
    uint32_t *counters = scratch.at<uint32_t>(tp + ti + arr);
    char *ws = scratch.at<char>(tp + ti + arr + cn);

    int rc = sblas_hip_csr_transpose_f64_i32(dev, stream, n, n, nnz, rowptr, colidx, nullptr, tptr, nnz > 0 ? tidx : nullptr, nullptr,
                                             nullptr, wsb > 0 ? ws : nullptr, wsb);
    if (rc != SBLAS_OK) return rc;
    const int32_t *dlist[3];
    {
        size_t at = 0;
        for (int t = 0; t < 3 && e == hipSuccess; ++t) {
            dlist[t] = list + at;
            if (!lists[t].empty()) e = hipMemcpyAsync(list + at, lists[t].data(), lists[t].size() * 4, hipMemcpyHostToDevice, s);
            at += lists[t].size();
        }
    }
    if (e == hipSuccess) e = hipMemsetAsync(p->color, 0xff, (size_t)n * 4, s); // every vertex -1
    if (e != hipSuccess) return SBLAS_E_HIP;

    const uint32_t salt = color_salt(seed);
    int64_t left = n;
    for (int batch = 4; left > 0; batch = batch * 2 < ROUND_BATCH_MAX ? batch * 2 : ROUND_BATCH_MAX) {
        e = hipMemsetAsync(counters, 0, cn, s);
        for (int r = 0; r < batch && e == hipSuccess; ++r) {
            for (int t = 0; t < 3; ++t) {
                const int64_t count = (int64_t)lists[t].size(), shift = 2 + 2 * t;
                if (count == 0) continue;
                const unsigned grid = (unsigned)(((count << shift) + COLOR_THREADS - 1) / COLOR_THREADS);
                if (t == 0)
                    color_round_kernel<2><<<grid, COLOR_THREADS, 0, s>>>(count, dlist[t], rowptr, colidx, tptr, tidx, salt, p->color, counters + r);
                else if (t == 1)
                    color_round_kernel<4><<<grid, COLOR_THREADS, 0, s>>>(count, dlist[t], rowptr, colidx, tptr, tidx, salt, p->color, counters + r);
                else
                    color_round_kernel<6><<<grid, COLOR_THREADS, 0, s>>>(count, dlist[t], rowptr, colidx, tptr, tidx, salt, p->color, counters + r);
            }
            e = hipGetLastError();
        }
        uint32_t h_counters[ROUND_BATCH_MAX];
        if (e == hipSuccess) e = hipMemcpyAsync(h_counters, counters, (size_t)batch * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s); // the host vectors of the lists are read until the first one
        if (e != hipSuccess) return SBLAS_E_HIP;
        for (int r = 0; r < batch && left > 0; ++r) {
            if (h_counters[r] == 0 || (int64_t)h_counters[r] > left) return SBLAS_E_INTERNAL; // no progress: never spin
            left -= h_counters[r];
            ++p->rounds;
        }
    }

    // the order: a stable sort of the colours with the vertex as payload
    const int32_t *skeys = p->color, *sidx = nullptr;
    {
        Workspace w;
        workspace_layout(n, ws, &w);
        const int passes = radix_passes(color_bound);
        for (int q = 0; q < passes; ++q) {
            if (radix_pass(s, w, skeys, sidx, n, q * RADIX_BITS, q & 1) != hipSuccess) return SBLAS_E_HIP;
            skeys = w.keys[q & 1], sidx = w.idx[q & 1];
        }
    }
    color_order_kernel<<<grid_for(n), T_THREADS, 0, s>>>(sidx, n, p->perm, p->inv);
    int32_t top = 0;
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&top, skeys + (n - 1), 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return SBLAS_E_HIP;
    if (top < 0 || (int64_t)top >= color_bound) return SBLAS_E_INTERNAL;
    p->colors = (int64_t)top + 1;
    colptr_kernel<<<grid_for(p->colors + 1), T_THREADS, 0, s>>>(skeys, n, p->colors, nullptr, p->color_ptr);
    std::vector<int32_t> h_ptr((size_t)p->colors + 1);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h_ptr.data(), p->color_ptr, h_ptr.size() * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return SBLAS_E_HIP;
    p->smallest = n;
    for (int64_t c = 0; c < p->colors; ++c) {
        const int64_t size = (int64_t)h_ptr[(size_t)c + 1] - h_ptr[(size_t)c];
        p->largest = size > p->largest ? size : p->largest;
        p->smallest = size < p->smallest ? size : p->smallest;
    }
    *plan_out = p.release();
    return SBLAS_OK;
}

int sblas_hip_color_plan_info(const void *plan, int64_t out[8])
{
    if (!plan || !out) return SBLAS_E_INVALID;
    const ColorPlan *p = static_cast<const ColorPlan *>(plan);
    out[0] = p->n, out[1] = p->nnz, out[2] = p->colors, out[3] = p->rounds, out[4] = p->largest, out[5] = p->smallest;
    out[6] = p->degree, out[7] = (int64_t)p->bytes;
    return SBLAS_OK;
}

int sblas_hip_color_plan_order(const void *plan, const int32_t **color, const int32_t **perm, const int32_t **inv,
                               const int32_t **color_ptr)
{
    if (!plan) return SBLAS_E_INVALID;
    const ColorPlan *p = static_cast<const ColorPlan *>(plan);
    if (color) *color = p->color;
    if (perm) *perm = p->perm;
    if (inv) *inv = p->inv;
    if (color_ptr) *color_ptr = p->color_ptr;
    return SBLAS_OK;
}

int sblas_hip_color_plan_destroy(void *plan)
{
    delete static_cast<ColorPlan *>(plan);
    return SBLAS_OK;
}

int sblas_hip_permute_plan_create(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                                  const int32_t *perm, void **plan_out, int64_t *bad)
{
    if (bad) *bad = -1;
    if (!plan_out) return SBLAS_E_INVALID;
    *plan_out = nullptr;
    if (n < 0 || nnz < 0 || n > INT_MAX - 64 || nnz > INT_MAX) return SBLAS_E_INVALID;
    if (n > 0 && (!rowptr || !perm)) return SBLAS_E_INVALID;
    if (nnz > 0 && (n == 0 || !colidx)) return SBLAS_E_INVALID;
    std::unique_ptr<PermutePlan> p(new PermutePlan);
    p->dev = resolve_device(dev), p->n = n, p->nnz = nnz;
    if (n > 0) {
        // the relabel kernel never sees a row pointer or a column outside the matrix
        const int vrc = sblas_hip_debug_validate_csr_i32(dev, stream, n, n, nnz, rowptr, colidx);
        if (vrc) return vrc;
    }
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    hipStream_t s = (hipStream_t)stream;
    DeviceBuffer triplets; // freed when B's structure stands
    int32_t *trow = nullptr, *tcol = nullptr;
    if (n > 0) {
        const size_t iv = align16((size_t)n * 4), word = 16;
        if (p->buf.alloc(p->dev, iv + word) != hipSuccess) return SBLAS_E_HIP;
        p->bytes = iv + word;
        p->inv = p->buf.at<int32_t>();
        int32_t *d_bad = p->buf.at<int32_t>(iv);
        int32_t h_bad = INT_MAX;
        hipError_t e = hipMemcpyAsync(d_bad, &h_bad, 4, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) {
            permute_fill_kernel<<<grid_for(n), T_THREADS, 0, s>>>(n, INT_MAX, p->inv); // above every index
            permute_first_kernel<<<grid_for(n), T_THREADS, 0, s>>>(n, perm, p->inv, d_bad);
            permute_repeat_kernel<<<grid_for(n), T_THREADS, 0, s>>>(n, perm, p->inv, d_bad);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return SBLAS_E_HIP;
        if (h_bad != INT_MAX) { // n entries of [0, n) without a repeat are a permutation
            if (bad) *bad = h_bad;
            return SBLAS_E_INVALID;
        }
        if (nnz > 0) {
            const size_t tr = align16((size_t)nnz * 4);
            if (triplets.alloc(p->dev, 2 * tr) != hipSuccess) return SBLAS_E_HIP;
            trow = triplets.at<int32_t>(), tcol = triplets.at<int32_t>(tr);
            permute_relabel_kernel<<<grid_for(nnz), T_THREADS, 0, s>>>(nnz, n, rowptr, colidx, p->inv, trow, tcol);
            if (hipGetLastError() != hipSuccess) return SBLAS_E_HIP;
        }
    }
    const int rc = sblas_hip_coo_plan_create(dev, stream, n, n, nnz, trow, tcol, SBLAS_COO_KEEP, &p->coo); // synchronises
    if (rc != SBLAS_OK) return rc;
    if (hipStreamSynchronize(s) != hipSuccess) return SBLAS_E_HIP;
    int64_t ci[8];
    if (sblas_hip_coo_plan_info(p->coo, ci) != SBLAS_OK) return SBLAS_E_INTERNAL;
    p->bytes += (size_t)ci[6];
    if (sblas_hip_coo_plan_csr(p->coo, nullptr, nullptr, &p->src, nullptr) != SBLAS_OK) return SBLAS_E_INTERNAL;
    *plan_out = p.release();
    return SBLAS_OK;
}

int sblas_hip_permute_plan_info(const void *plan, int64_t out[4])
{
    if (!plan || !out) return SBLAS_E_INVALID;
    const PermutePlan *p = static_cast<const PermutePlan *>(plan);
    int64_t ci[8] = {0};
    if (sblas_hip_coo_plan_info(p->coo, ci) != SBLAS_OK) return SBLAS_E_INTERNAL;
    out[0] = p->n, out[1] = p->nnz, out[2] = ci[5], out[3] = (int64_t)p->bytes;
    return SBLAS_OK;
}

int sblas_hip_permute_plan_csr(const void *plan, const int32_t **rowptr_b, const int32_t **colidx_b, const int32_t **src)
{
    if (!plan) return SBLAS_E_INVALID;
    return sblas_hip_coo_plan_csr(static_cast<const PermutePlan *>(plan)->coo, rowptr_b, colidx_b, src, nullptr);
}

int sblas_hip_permute_plan_inverse(const void *plan, const int32_t **inv)
{
    if (!plan || !inv) return SBLAS_E_INVALID;
    *inv = static_cast<const PermutePlan *>(plan)->inv;
    return SBLAS_OK;
}

int sblas_hip_permute_plan_values(const void *plan, void *stream, const double *val_a, double *val_b)
{
    if (!plan) return SBLAS_E_INVALID;
    const PermutePlan *p = static_cast<const PermutePlan *>(plan);
    if (p->nnz == 0) return SBLAS_OK;
    if (!val_a || !val_b) return SBLAS_E_INVALID;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID; // the plan's arrays live on its own device
    gather_f64_kernel<<<grid_for(p->nnz), T_THREADS, 0, (hipStream_t)stream>>>(p->nnz, p->src, val_a, val_b);
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_permute_plan_destroy(void *plan)
{
    delete static_cast<PermutePlan *>(plan);
    return SBLAS_OK;
}

} // extern "C"
