// spgemm.hip -- C = A * B for two CSR matrices on the device (sblas_hip_spgemm_plan_*): create does the symbolic work
// once and owns C's rowptr and colidx, numeric fills C's values for new values of A and B.  The contract ((S), (V), (I),
// (D)) stands above the declarations in sblas_hip.h; the host rule that sends each row to a path is spgemm_plan.cpp.
//
// The row path (B's rows strictly ascending, the row's column span <= SPGEMM_S_MAX).  A workgroup is one wave; the wave,
// or each of its four 16-lane groups, owns one row of C from start to end.  It walks the row's A entries one at a time in
// stored order -- their columns, values and B row bounds fetched a group's width ahead and handed round by shuffles --
// and the lanes spread across the named B row, whose indices and values stream from memory coalesced.  Because a B row
// has no column twice, the lanes of one step touch distinct entries of C: the order of (V) is the order of the steps.
//   symbolic  a bitmap in LDS over [lo, hi], lo / hi the least first and greatest last column of the named B rows, set
//             with 32-bit atomicOr (which lane sets a bit first changes nothing); the popcounts give the row's count, and
//             after the scan of the counts a second walk rebuilds the bitmap and writes colidx_C ascending;
//   numeric   the bitmap is rebuilt from colidx_C (no B row is read for it), an exclusive popcount prefix of its words is
//             kept beside it, and an entry's place in the row is prefix[word] + popcount(bits below it).  The
//             accumulators start at -0.0, the identity of fp64 addition for every operand (x + -0.0 has the bits of x
//             for every x that is not a NaN, -0.0 included), so the first product arrives as if copied and every later
//             one is one plain add.  They live in LDS while the C row fits (SPGEMM_ACC_CAP entries; a quarter of it for
//             a narrow group) and in val_C itself beyond that.
// Step order.  LDS: a wave's LDS instructions execute in issue order, so a wavefront-scope fence (which only keeps the
// compiler from moving accesses across it) is enough for a later step to read what an earlier step wrote.  val_C: the
// owning wave is the only writer; every step ends with a workgroup-scope acquire-release fence and a wait for the
// step's stores (vmcnt(0)) before the next step's loads are issued, and both go through the wave's own CU.
//
// The general path (every other row, or all of them under SBLAS_SPGEMM_GENERAL): the chunks of spgemm_plan.cpp, each
// expanded into triplets (local row, column, a * b) in the numbering of (V) -- one thread per product, which finds its A
// entry by a binary search in the exclusive scan of the named B rows' lengths -- then sorted and run-summed by coo.hip's
// own passes (coo_sum.h) into a chunk-local CSR and copied to its rows of C.  numeric sorts again on every call: the
// workspace is sized by the largest chunk, not by the product count.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <memory>
#include <vector>
#include "../../include/sblas_hip.h"
#include "capi_util.h"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function" // radix_sort.h's value gather: the transpose's, not used here
#include "coo_sum.h"
#pragma clang diagnostic pop
#include "spgemm.h"

// a * b and acc + p are separate roundings
#pragma clang fp contract(off)

namespace {

using sblas::SPGEMM_ACC_CAP;
using sblas::SPGEMM_S_MAX;

constexpr int ROW_WORDS = (int)(SPGEMM_S_MAX / 32); // bitmap words of one wave
constexpr int SG = 8;                               // lanes per row of the structure passes (analyse, check, copy)

// rowptr[0] == 0 and no step down: flag |= 1
__global__ __launch_bounds__(T_THREADS) void rowptr_check_kernel(int64_t rows, const int32_t *__restrict__ rowptr, int *__restrict__ flag)
{
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * T_THREADS + threadIdx.x; i < rows; i += (int64_t)gridDim.x * T_THREADS) {
        if (rowptr[i + 1] < rowptr[i]) bad = 1;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && rowptr[0] != 0) bad = 1;
    if (bad) atomicOr(flag, 1);
}

// a column outside [0, cols): flag |= 1
__global__ __launch_bounds__(T_THREADS) void colidx_check_kernel(int64_t nnz, int64_t cols, const int32_t *__restrict__ colidx, int *__restrict__ flag)
{
    int bad = 0;
    for (int64_t p = (int64_t)blockIdx.x * T_THREADS + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * T_THREADS) {
        const int32_t c = colidx[p];
        if (c < 0 || (int64_t)c >= cols) bad = 1;
    }
    if (bad) atomicOr(flag, 1);
}

// a row of B that is not strictly ascending: flag |= 1.  Eight lanes a row.
__global__ __launch_bounds__(T_THREADS) void ascending_check_kernel(int64_t rows, const int32_t *__restrict__ rowptr,
                                                                    const int32_t *__restrict__ colidx, int *__restrict__ flag)
{
    const int lane = threadIdx.x & (SG - 1);
    int bad = 0;
    for (int64_t i = ((int64_t)blockIdx.x * T_THREADS + threadIdx.x) / SG; i < rows; i += (int64_t)gridDim.x * (T_THREADS / SG)) {
        const int32_t b0 = rowptr[i], b1 = rowptr[i + 1];
        for (int32_t p = b0 + 1 + lane; p < b1; p += SG)
            if (colidx[p] <= colidx[p - 1]) bad = 1;
    }
    if (bad) atomicOr(flag, 1);
}

// products[i] = the stored entries of the B rows that A's row i names, one count per stored a_ik; span[i] = the columns
// from the least first to the greatest last column of those rows (0 when all are empty; the true span when B's rows
// are ascending, not used otherwise).  Eight lanes a row.
__global__ __launch_bounds__(T_THREADS) void analyse_kernel(int64_t m, const int32_t *__restrict__ rowptr_a,
                                                            const int32_t *__restrict__ colidx_a, const int32_t *__restrict__ rowptr_b,
                                                            const int32_t *__restrict__ colidx_b, int64_t *__restrict__ products,
                                                            int64_t *__restrict__ span)
{
    const int lane = threadIdx.x & (SG - 1);
    for (int64_t i = ((int64_t)blockIdx.x * T_THREADS + threadIdx.x) / SG; i < m; i += (int64_t)gridDim.x * (T_THREADS / SG)) {
        long long sum = 0;
        int lo = INT_MAX, hi = -1;
        for (int32_t e = rowptr_a[i] + lane, a1 = rowptr_a[i + 1]; e < a1; e += SG) {
            const int32_t k = colidx_a[e], b0 = rowptr_b[k], b1 = rowptr_b[k + 1];
            sum += b1 - b0;
            if (b1 > b0) {
                const int32_t f = colidx_b[b0], l = colidx_b[b1 - 1];
                lo = f < lo ? f : lo, hi = l > hi ? l : hi;
            }
        }
        for (int o = SG / 2; o > 0; o >>= 1) {
            sum += __shfl_xor(sum, o, SG);
            const int l2 = __shfl_xor(lo, o, SG), h2 = __shfl_xor(hi, o, SG);
            lo = l2 < lo ? l2 : lo, hi = h2 > hi ? h2 : hi;
        }
        if (lane == 0) products[i] = sum, span[i] = hi >= lo ? (int64_t)hi - lo + 1 : 0;
    }
}

// total += the n counts (integer: the same whatever the order)
__global__ __launch_bounds__(T_THREADS) void sum_counts_kernel(int64_t n, const uint32_t *__restrict__ cnt, unsigned long long *__restrict__ total)
{
    unsigned long long s = 0;
    for (int64_t i = (int64_t)blockIdx.x * T_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * T_THREADS) s += cnt[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(total, s);
}

// ----------------------------------------------------------------------------------------------------------------
// the row path
// ----------------------------------------------------------------------------------------------------------------

// a later LDS access of this wave sees an earlier one: LDS instructions execute in issue order, the fence keeps the
// compiler from reordering them
__device__ inline void lds_step_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// a later load of this wave sees an earlier store of it to val_C: the workgroup-scope fence orders them (the vector
// memory path of one CU performs a workgroup's accesses in order, so on this target the fence alone emits no wait for
// them); the explicit wait makes the step's stores complete before the next step's loads are issued in any case
__device__ inline void mem_step_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// Sets the bit of every column of C's row in the group's bitmap (cleared here), from A's row [a0, a1) and the B rows it
// names.  lo: the row's least column.
template <int G>
__device__ inline void mark_row(uint32_t *bits, int words, int lane, int32_t a0, int32_t a1, int32_t lo,
                                const int32_t *__restrict__ colidx_a, const int32_t *__restrict__ rowptr_b,
                                const int32_t *__restrict__ colidx_b)
{
    for (int w = lane; w < words; w += G) bits[w] = 0u;
    lds_step_sync();
    for (int32_t e0 = a0; e0 < a1; e0 += G) {
        const bool live = e0 + lane < a1;
        const int32_t k = live ? colidx_a[e0 + lane] : 0;
        const int32_t rb0 = live ? rowptr_b[k] : 0, rb1 = live ? rowptr_b[k + 1] : 0;
        const int cnt = a1 - e0 < G ? a1 - e0 : G;
        for (int j = 0; j < cnt; ++j) {
            const int32_t b0 = __shfl(rb0, j, G), b1 = __shfl(rb1, j, G);
            for (int32_t f = b0 + lane; f < b1; f += G) {
                const uint32_t c = (uint32_t)(colidx_b[f] - lo);
                atomicOr(&bits[c >> 5], 1u << (c & 31u));
            }
        }
    }
    lds_step_sync();
}

// least first / greatest last column of the B rows that A's row names (some row is not empty: the row has products)
template <int G>
__device__ inline void row_bounds(int lane, int32_t a0, int32_t a1, const int32_t *__restrict__ colidx_a,
                                  const int32_t *__restrict__ rowptr_b, const int32_t *__restrict__ colidx_b, int32_t *lo_out,
                                  int32_t *hi_out)
{
    int lo = INT_MAX, hi = -1;
    for (int32_t e = a0 + lane; e < a1; e += G) {
        const int32_t k = colidx_a[e], b0 = rowptr_b[k], b1 = rowptr_b[k + 1];
        if (b1 > b0) {
            const int32_t f = colidx_b[b0], l = colidx_b[b1 - 1];
            lo = f < lo ? f : lo, hi = l > hi ? l : hi;
        }
    }
    for (int o = G / 2; o > 0; o >>= 1) {
        const int l2 = __shfl_xor(lo, o, G), h2 = __shfl_xor(hi, o, G);
        lo = l2 < lo ? l2 : lo, hi = h2 > hi ? h2 : hi;
    }
    *lo_out = lo, *hi_out = hi;
}

// inclusive sum of v over the group's lanes
template <int G> __device__ inline uint32_t group_inclusive_scan(uint32_t v, int lane)
{
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < G; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, G);
        if (lane >= o) x += y;
    }
    return x;
}

// FILL == false: counts[i] = the entries of C's row i.  FILL == true: colidx_c[rowptr_c[i] ...] = its columns, ascending.
// One wave a workgroup, 64 / G rows a wave.
template <int G, bool FILL>
__global__ __launch_bounds__(64) void row_symbolic_kernel(int64_t nrows, const int32_t *__restrict__ rows,
                                                          const int32_t *__restrict__ rowptr_a, const int32_t *__restrict__ colidx_a,
                                                          const int32_t *__restrict__ rowptr_b, const int32_t *__restrict__ colidx_b,
                                                          uint32_t *counts, const int32_t *rowptr_c, int32_t *__restrict__ colidx_c)
{
    constexpr int NG = 64 / G, WORDS = ROW_WORDS / NG;
    __shared__ uint32_t s_bits[ROW_WORDS];
    const int lane = threadIdx.x & (G - 1), grp = threadIdx.x / G;
    uint32_t *bits = s_bits + grp * WORDS;
    for (int64_t r = (int64_t)blockIdx.x * NG + grp; r < nrows; r += (int64_t)gridDim.x * NG) {
        const int32_t i = rows[r], a0 = rowptr_a[i], a1 = rowptr_a[i + 1];
        int32_t lo, hi;
        row_bounds<G>(lane, a0, a1, colidx_a, rowptr_b, colidx_b, &lo, &hi);
        const int words = ((hi - lo) >> 5) + 1; // <= WORDS: the host rule sends wider rows elsewhere
        mark_row<G>(bits, words, lane, a0, a1, lo, colidx_a, rowptr_b, colidx_b);
        uint32_t carry = 0;
        for (int w0 = 0; w0 < words; w0 += G) {
            const int w = w0 + lane;
            uint32_t b = w < words ? bits[w] : 0u;
            const uint32_t v = (uint32_t)__popc(b), x = group_inclusive_scan<G>(v, lane);
            if (FILL) {
                int32_t p = rowptr_c[i] + (int32_t)(carry + x - v);
                for (; b; b &= b - 1u) colidx_c[p++] = lo + w * 32 + (__ffs((int)b) - 1);
            }
            carry += __shfl(x, G - 1, G);
        }
        if (!FILL && lane == 0) counts[i] = carry;
        lds_step_sync(); // the next row clears the bitmap
    }
}

// val_c's row i = the products of A's row i, accumulated in the numbering of (V).  One wave a workgroup, 64 / G rows a wave.
template <int G>
__global__ __launch_bounds__(64) void row_numeric_kernel(int64_t nrows, const int32_t *__restrict__ rows,
                                                         const int32_t *__restrict__ rowptr_a, const int32_t *__restrict__ colidx_a,
                                                         const double *__restrict__ val_a, const int32_t *__restrict__ rowptr_b,
                                                         const int32_t *__restrict__ colidx_b, const double *__restrict__ val_b,
                                                         const int32_t *__restrict__ rowptr_c, const int32_t *__restrict__ colidx_c,
                                                         double *val_c)
{
    constexpr int NG = 64 / G, WORDS = ROW_WORDS / NG, ACC = (int)(SPGEMM_ACC_CAP / NG);
    __shared__ uint32_t s_bits[ROW_WORDS];
    __shared__ uint32_t s_pre[ROW_WORDS];
    __shared__ double s_acc[SPGEMM_ACC_CAP];
    const int lane = threadIdx.x & (G - 1), grp = threadIdx.x / G;
    uint32_t *bits = s_bits + grp * WORDS, *pre = s_pre + grp * WORDS;
    double *acc = s_acc + grp * ACC;
    for (int64_t r = (int64_t)blockIdx.x * NG + grp; r < nrows; r += (int64_t)gridDim.x * NG) {
        const int32_t i = rows[r], c0 = rowptr_c[i], len = rowptr_c[i + 1] - c0;
        if (len <= 0) continue;
        const int32_t lo = colidx_c[c0], hi = colidx_c[c0 + len - 1]; // the row is ascending
        const int words = ((hi - lo) >> 5) + 1;
        for (int w = lane; w < words; w += G) bits[w] = 0u;
        lds_step_sync();
        for (int32_t j = lane; j < len; j += G) {
            const uint32_t c = (uint32_t)(colidx_c[c0 + j] - lo);
            atomicOr(&bits[c >> 5], 1u << (c & 31u));
        }
        lds_step_sync();
        uint32_t carry = 0;
        for (int w0 = 0; w0 < words; w0 += G) {
            const int w = w0 + lane;
            const uint32_t v = w < words ? (uint32_t)__popc(bits[w]) : 0u, x = group_inclusive_scan<G>(v, lane);
            if (w < words) pre[w] = carry + x - v;
            carry += __shfl(x, G - 1, G);
        }
        const bool in_lds = len <= ACC;
        if (in_lds) {
            for (int32_t j = lane; j < len; j += G) acc[j] = -0.0;
            lds_step_sync();
        } else {
            for (int32_t j = lane; j < len; j += G) val_c[c0 + j] = -0.0;
            mem_step_sync();
        }
        const int32_t a0 = rowptr_a[i], a1 = rowptr_a[i + 1];
        for (int32_t e0 = a0; e0 < a1; e0 += G) { // the next G entries of A's row, one to a lane
            const bool live = e0 + lane < a1;
            const int32_t k = live ? colidx_a[e0 + lane] : 0;
            const double av = live ? val_a[e0 + lane] : 0.0;
            const int32_t rb0 = live ? rowptr_b[k] : 0, rb1 = live ? rowptr_b[k + 1] : 0;
            const int cnt = a1 - e0 < G ? a1 - e0 : G;
            for (int j = 0; j < cnt; ++j) { // one step: a_ik times B's row k
                const int32_t b0 = __shfl(rb0, j, G), b1 = __shfl(rb1, j, G);
                const double a = __shfl(av, j, G);
                for (int32_t f = b0 + lane; f < b1; f += G) {
                    const uint32_t c = (uint32_t)(colidx_b[f] - lo), w = c >> 5;
                    const uint32_t pos = pre[w] + (uint32_t)__popc(bits[w] & ((1u << (c & 31u)) - 1u));
                    const double p = a * val_b[f];
                    if (in_lds) acc[pos] = acc[pos] + p;
                    else val_c[c0 + pos] = val_c[c0 + pos] + p;
                }
                if (in_lds) lds_step_sync();
                else mem_step_sync();
            }
        }
        if (in_lds) {
            for (int32_t j = lane; j < len; j += G) val_c[c0 + j] = acc[j];
            lds_step_sync(); // the next row clears the accumulators
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------
// the general path
// ----------------------------------------------------------------------------------------------------------------

// For the chunk's rows (rows[0 .. R), their A entries numbered from abase[r] on): aoff[q] = the length of the B row that
// A entry q names, apos[q] = the entry's position in A, arow[q] = its chunk-local row; aoff[NA] = 0.  Eight lanes a row.
__global__ __launch_bounds__(T_THREADS) void gen_lengths_kernel(int64_t R, int64_t NA, const int32_t *__restrict__ rows,
                                                                const int32_t *__restrict__ abase, const int32_t *__restrict__ rowptr_a,
                                                                const int32_t *__restrict__ colidx_a, const int32_t *__restrict__ rowptr_b,
                                                                uint32_t *__restrict__ aoff, int32_t *__restrict__ apos,
                                                                int32_t *__restrict__ arow)
{
    const int lane = threadIdx.x & (SG - 1);
    if (blockIdx.x == 0 && threadIdx.x == 0) aoff[NA] = 0u;
    for (int64_t r = ((int64_t)blockIdx.x * T_THREADS + threadIdx.x) / SG; r < R; r += (int64_t)gridDim.x * (T_THREADS / SG)) {
        const int32_t i = rows[r], a0 = rowptr_a[i], a1 = rowptr_a[i + 1], q0 = abase[r];
        for (int32_t e = a0 + lane; e < a1; e += SG) {
            const int32_t k = colidx_a[e], q = q0 + (e - a0);
            aoff[q] = (uint32_t)(rowptr_b[k + 1] - rowptr_b[k]);
            apos[q] = e, arow[q] = (int32_t)r;
        }
    }
}

// Product t of the chunk, in the numbering of (V): A entry q = the last one whose scanned offset is <= t (a binary
// search; entries that name an empty row share their successor's offset and are never found), B entry t - aoff[q] of
// the row it names.  pval == nullptr: the keys only.
__global__ __launch_bounds__(T_THREADS) void gen_expand_kernel(int64_t P, int64_t NA, const uint32_t *__restrict__ aoff,
                                                               const int32_t *__restrict__ apos, const int32_t *__restrict__ arow,
                                                               const int32_t *__restrict__ colidx_a, const double *__restrict__ val_a,
                                                               const int32_t *__restrict__ rowptr_b, const int32_t *__restrict__ colidx_b,
                                                               const double *__restrict__ val_b, int32_t *__restrict__ krow,
                                                               int32_t *__restrict__ kcol, double *__restrict__ pval)
{
    for (int64_t t = (int64_t)blockIdx.x * T_THREADS + threadIdx.x; t < P; t += (int64_t)gridDim.x * T_THREADS) {
        int64_t lo = 0, hi = NA;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)aoff[mid] <= t) lo = mid + 1;
            else hi = mid;
        }
        const int64_t q = lo - 1; // aoff[0] = 0 <= t
        const int32_t e = apos[q], k = colidx_a[e];
        const int64_t f = (int64_t)rowptr_b[k] + (t - (int64_t)aoff[q]);
        krow[t] = arow[q], kcol[t] = colidx_b[f];
        if (pval) pval[t] = val_a[e] * val_b[f];
    }
}

// counts[rows[r]] = the entries of the chunk-local row r
__global__ __launch_bounds__(T_THREADS) void gen_counts_kernel(int64_t R, const int32_t *__restrict__ rows, const int32_t *__restrict__ rowptr_loc,
                                                               uint32_t *__restrict__ counts)
{
    for (int64_t r = (int64_t)blockIdx.x * T_THREADS + threadIdx.x; r < R; r += (int64_t)gridDim.x * T_THREADS)
        counts[rows[r]] = (uint32_t)(rowptr_loc[r + 1] - rowptr_loc[r]);
}

// the chunk-local rows to their places in C.  Eight lanes a row.
template <typename T>
__global__ __launch_bounds__(T_THREADS) void gen_place_kernel(int64_t R, const int32_t *__restrict__ rows, const int32_t *__restrict__ rowptr_loc,
                                                              const T *__restrict__ src, const int32_t *__restrict__ rowptr_c, T *__restrict__ dst)
{
    const int lane = threadIdx.x & (SG - 1);
    for (int64_t r = ((int64_t)blockIdx.x * T_THREADS + threadIdx.x) / SG; r < R; r += (int64_t)gridDim.x * (T_THREADS / SG)) {
        const int32_t s0 = rowptr_loc[r], len = rowptr_loc[r + 1] - s0, d0 = rowptr_c[rows[r]];
        for (int32_t j = lane; j < len; j += SG) dst[d0 + j] = src[s0 + j];
    }
}

struct Chunk {
    int64_t g0, R, NA, P; // first general row (ordinal), rows, A entries, products
};

// the general path's workspace, laid out for the largest chunk in each measure
struct GenWork {
    void *coo = nullptr;
    int32_t *krow = nullptr, *kcol = nullptr, *apos = nullptr, *arow = nullptr, *rowptr_loc = nullptr, *colidx_loc = nullptr;
    uint32_t *aoff = nullptr, *abs = nullptr;
    double *pval = nullptr, *val_loc = nullptr;
};

size_t gen_layout(int64_t P, int64_t NA, int64_t R, char *base, GenWork *w)
{
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *p = base ? base + off : nullptr;
        off += align16(bytes);
        return p;
    };
    char *coo = take(coo_layout(P, nullptr, nullptr));
    char *krow = take((size_t)P * 4), *kcol = take((size_t)P * 4), *pval = take((size_t)P * 8);
    char *aoff = take(((size_t)NA + 1) * 4), *abs = take((size_t)ceil_div(NA + 1, SCAN_TILE) * 4);
    char *apos = take((size_t)NA * 4 + 4), *arow = take((size_t)NA * 4 + 4);
    char *rl = take(((size_t)R + 1) * 4), *cl = take((size_t)P * 4), *vl = take((size_t)P * 8);
    if (w) {
        w->coo = coo, w->krow = (int32_t *)krow, w->kcol = (int32_t *)kcol, w->pval = (double *)pval;
        w->aoff = (uint32_t *)aoff, w->abs = (uint32_t *)abs, w->apos = (int32_t *)apos, w->arow = (int32_t *)arow;
        w->rowptr_loc = (int32_t *)rl, w->colidx_loc = (int32_t *)cl, w->val_loc = (double *)vl;
    }
    return off;
}

struct SpgemmPlan {
    int dev = -1, flags = 0;
    int64_t m = 0, k = 0, n = 0, nnz_a = 0, nnz_b = 0, nnz_c = 0, products = 0, rows64 = 0, rows16 = 0, rows_general = 0;
    int64_t max_row_products = 0, b_ascending = 0;
    size_t bytes = 0;
    DeviceBuffer structure; // rowptr_a | colidx_a | rowptr_b | colidx_b: the plan's own copies
    DeviceBuffer rowptr_buf, colidx_buf, lists, work;
    int32_t *rowptr_a = nullptr, *colidx_a = nullptr, *rowptr_b = nullptr, *colidx_b = nullptr;
    int32_t *rowptr_c = nullptr, *colidx_c = nullptr;
    int32_t *list64 = nullptr, *list16 = nullptr, *gen_rows = nullptr, *gen_abase = nullptr;
    std::vector<Chunk> chunks;
    GenWork gw;
};

inline unsigned row_grid(int64_t nrows, int per_wave)
{
    const int64_t b = ceil_div(nrows, per_wave);
    return (unsigned)(b < 1 ? 1 : b > (1 << 20) ? (1 << 20) : b);
}
inline unsigned sg_grid(int64_t rows) { return grid_for(rows * SG); }

// One chunk through expand, sort and run-sum into the chunk-local CSR (rowptr_loc, colidx_loc and, with values, val_loc).
hipError_t run_chunk(const SpgemmPlan &p, hipStream_t s, const Chunk &c, const double *val_a, const double *val_b)
{
    const GenWork &w = p.gw;
    const int32_t *rows = p.gen_rows + c.g0, *abase = p.gen_abase + c.g0;
    gen_lengths_kernel<<<sg_grid(c.R), T_THREADS, 0, s>>>(c.R, c.NA, rows, abase, p.rowptr_a, p.colidx_a, p.rowptr_b, w.aoff, w.apos, w.arow);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = scan_exclusive(s, w.aoff, c.NA + 1, w.abs, ceil_div(c.NA + 1, SCAN_TILE));
    if (e != hipSuccess) return e;
    gen_expand_kernel<<<grid_for(c.P), T_THREADS, 0, s>>>(c.P, c.NA, w.aoff, w.apos, w.arow, p.colidx_a, val_a, p.rowptr_b, p.colidx_b, val_b,
                                                         w.krow, w.kcol, val_a ? w.pval : nullptr);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return run_coo(s, c.R, p.n, c.P, w.krow, w.kcol, val_a ? w.pval : nullptr, SBLAS_COO_SUM, w.rowptr_loc, w.colidx_loc,
                   val_a ? w.val_loc : nullptr, nullptr, nullptr, w.coo);
}

template <bool FILL> hipError_t launch_symbolic(const SpgemmPlan &p, hipStream_t s, uint32_t *counts)
{
    if (p.rows64 > 0)
        row_symbolic_kernel<64, FILL><<<row_grid(p.rows64, 1), 64, 0, s>>>(p.rows64, p.list64, p.rowptr_a, p.colidx_a, p.rowptr_b, p.colidx_b,
                                                                          counts, p.rowptr_c, p.colidx_c);
    if (p.rows16 > 0)
        row_symbolic_kernel<sblas::SPGEMM_NARROW, FILL><<<row_grid(p.rows16, 64 / sblas::SPGEMM_NARROW), 64, 0, s>>>(
            p.rows16, p.list16, p.rowptr_a, p.colidx_a, p.rowptr_b, p.colidx_b, counts, p.rowptr_c, p.colidx_c);
    hipError_t e = hipGetLastError();
    for (size_t c = 0; c < p.chunks.size() && e == hipSuccess; ++c) {
        const Chunk &ch = p.chunks[c];
        e = run_chunk(p, s, ch, nullptr, nullptr);
        if (e != hipSuccess) break;
        if (FILL)
            gen_place_kernel<int32_t><<<sg_grid(ch.R), T_THREADS, 0, s>>>(ch.R, p.gen_rows + ch.g0, p.gw.rowptr_loc, p.gw.colidx_loc, p.rowptr_c,
                                                                          p.colidx_c);
        else
            gen_counts_kernel<<<grid_for(ch.R), T_THREADS, 0, s>>>(ch.R, p.gen_rows + ch.g0, p.gw.rowptr_loc, counts);
        e = hipGetLastError();
    }
    return e;
}

// rowptr (rows + 1 entries) starts at 0 and never steps down; *nnz = rowptr[rows]
hipError_t check_rowptr(hipStream_t s, int64_t rows, const int32_t *rowptr, int *flag, int *bad, int32_t *nnz)
{
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), s);
    if (e != hipSuccess) return e;
    rowptr_check_kernel<<<grid_for(rows), T_THREADS, 0, s>>>(rows, rowptr, flag);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(bad, flag, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(nnz, rowptr + rows, sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
}

hipError_t check_colidx(hipStream_t s, int64_t nnz, int64_t cols, const int32_t *colidx, int *flag, int *bad)
{
    *bad = 0;
    if (nnz == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), s);
    if (e != hipSuccess) return e;
    colidx_check_kernel<<<grid_for(nnz), T_THREADS, 0, s>>>(nnz, cols, colidx, flag);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(bad, flag, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
}

} // namespace

extern "C" {

int sblas_hip_spgemm_plan_create(int dev, void *stream, int64_t m, int64_t k, int64_t n, const int32_t *rowptr_a,
                                 const int32_t *colidx_a, const int32_t *rowptr_b, const int32_t *colidx_b, int flags,
                                 int64_t chunk_cap, void **plan_out)
{
    if (!plan_out) return SBLAS_E_INVALID;
    *plan_out = nullptr;
    if (m < 0 || k < 0 || n < 0 || m > INT_MAX || k > INT_MAX || n > INT_MAX || chunk_cap < 0) return SBLAS_E_INVALID;
    if (flags != SBLAS_SPGEMM_AUTO && flags != SBLAS_SPGEMM_GENERAL) return SBLAS_E_INVALID;
    if (!rowptr_a || !rowptr_b) return SBLAS_E_INVALID;
    std::unique_ptr<SpgemmPlan> p(new SpgemmPlan);
    p->dev = resolve_device(dev), p->flags = flags, p->m = m, p->k = k, p->n = n;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    hipStream_t s = (hipStream_t)stream;

    // the checks: nothing follows an index before it is known to be in range
    DeviceBuffer small; // [0] a flag, [2..3] a 64-bit total
    if (small.alloc(p->dev, 16) != hipSuccess) return SBLAS_E_HIP;
    int *flag = small.at<int>();
    int bad = 0;
    int32_t nnz_a = 0, nnz_b = 0;
    if (check_rowptr(s, m, rowptr_a, flag, &bad, &nnz_a) != hipSuccess) return SBLAS_E_HIP;
    if (bad) return SBLAS_E_INVALID;
    if (check_rowptr(s, k, rowptr_b, flag, &bad, &nnz_b) != hipSuccess) return SBLAS_E_HIP;
    if (bad) return SBLAS_E_INVALID;
    if ((nnz_a > 0 && !colidx_a) || (nnz_b > 0 && !colidx_b)) return SBLAS_E_INVALID;
    if (check_colidx(s, nnz_a, k, colidx_a, flag, &bad) != hipSuccess) return SBLAS_E_HIP;
    if (bad) return SBLAS_E_INVALID;
    if (check_colidx(s, nnz_b, n, colidx_b, flag, &bad) != hipSuccess) return SBLAS_E_HIP;
    if (bad) return SBLAS_E_INVALID;
    p->nnz_a = nnz_a, p->nnz_b = nnz_b;

    // the plan's own copy of both structures: numeric takes values only
    const size_t ra = align16(((size_t)m + 1) * 4), ca = align16((size_t)nnz_a * 4 + 4), rb = align16(((size_t)k + 1) * 4),
                 cb = align16((size_t)nnz_b * 4 + 4);
    if (p->structure.alloc(p->dev, ra + ca + rb + cb) != hipSuccess) return SBLAS_E_HIP;
    p->rowptr_a = p->structure.at<int32_t>(), p->colidx_a = p->structure.at<int32_t>(ra);
    p->rowptr_b = p->structure.at<int32_t>(ra + ca), p->colidx_b = p->structure.at<int32_t>(ra + ca + rb);
    hipError_t e = hipMemcpyAsync(p->rowptr_a, rowptr_a, ((size_t)m + 1) * 4, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && nnz_a > 0) e = hipMemcpyAsync(p->colidx_a, colidx_a, (size_t)nnz_a * 4, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(p->rowptr_b, rowptr_b, ((size_t)k + 1) * 4, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && nnz_b > 0) e = hipMemcpyAsync(p->colidx_b, colidx_b, (size_t)nnz_b * 4, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return SBLAS_E_HIP;
    p->bytes = ra + ca + rb + cb;

    // C's row pointers; until the scan they hold the rows' counts
    const size_t rc = align16(((size_t)m + 1) * 4);
    if (p->rowptr_buf.alloc(p->dev, rc) != hipSuccess) return SBLAS_E_HIP;
    p->rowptr_c = p->rowptr_buf.at<int32_t>();
    p->bytes += rc;
    if (hipMemsetAsync(p->rowptr_c, 0, ((size_t)m + 1) * 4, s) != hipSuccess) return SBLAS_E_HIP;

    // one pass over A's rows: products and spans; one over B's columns: ascending or not
    std::vector<int64_t> products((size_t)m), span((size_t)m), chunk_first((size_t)m + 1);
    std::vector<int32_t> h_rowptr_a((size_t)m + 1);
    std::vector<uint8_t> path((size_t)m);
    if (m > 0) {
        DeviceBuffer stats;
        if (stats.alloc(p->dev, (size_t)m * 16) != hipSuccess) return SBLAS_E_HIP;
        int64_t *d_products = stats.at<int64_t>(), *d_span = stats.at<int64_t>((size_t)m * 8);
        e = hipMemsetAsync(flag, 0, sizeof(int), s);
        if (e == hipSuccess) {
            ascending_check_kernel<<<sg_grid(k), T_THREADS, 0, s>>>(k, p->rowptr_b, p->colidx_b, flag);
            analyse_kernel<<<sg_grid(m), T_THREADS, 0, s>>>(m, p->rowptr_a, p->colidx_a, p->rowptr_b, p->colidx_b, d_products, d_span);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(products.data(), d_products, (size_t)m * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(span.data(), d_span, (size_t)m * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(h_rowptr_a.data(), p->rowptr_a, ((size_t)m + 1) * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return SBLAS_E_HIP;
        p->b_ascending = bad ? 0 : 1;
    } else {
        p->b_ascending = 1; // no row of C asks
    }

    // the host rule, then the row lists
    int64_t n_chunks = 0;
    if (sblas_hip_spgemm_classify(m, products.data(), span.data(), (int)p->b_ascending, flags, chunk_cap, path.data(), chunk_first.data(),
                                  &n_chunks) != SBLAS_OK)
        return SBLAS_E_INVALID;
    std::vector<int32_t> l64, l16, gen, gen_abase;
    for (int64_t i = 0; i < m; ++i) {
        p->products += products[i];
        p->max_row_products = products[i] > p->max_row_products ? products[i] : p->max_row_products;
        if (path[i] == SBLAS_SPGEMM_PATH_ROW) {
            const int g = sblas_hip_spgemm_group_width(products[i], (int64_t)h_rowptr_a[i + 1] - h_rowptr_a[i], span[i]);
            (g == 64 ? l64 : l16).push_back((int32_t)i);
        } else if (path[i] == SBLAS_SPGEMM_PATH_GENERAL) {
            if (products[i] > INT_MAX) return SBLAS_E_INVALID; // one row's triplets are sorted in one piece, with int32 positions
            gen.push_back((int32_t)i);
        }
    }
    p->rows64 = (int64_t)l64.size(), p->rows16 = (int64_t)l16.size(), p->rows_general = (int64_t)gen.size();
    gen_abase.resize(gen.size());
    int64_t maxP = 0, maxNA = 0, maxR = 0;
    for (int64_t c = 0; c < n_chunks; ++c) {
        Chunk ch{chunk_first[c], chunk_first[c + 1] - chunk_first[c], 0, 0};
        for (int64_t g = ch.g0; g < ch.g0 + ch.R; ++g) {
            const int32_t i = gen[g];
            gen_abase[g] = (int32_t)ch.NA;
            ch.NA += h_rowptr_a[i + 1] - h_rowptr_a[i], ch.P += products[i];
        }
        maxP = ch.P > maxP ? ch.P : maxP, maxNA = ch.NA > maxNA ? ch.NA : maxNA, maxR = ch.R > maxR ? ch.R : maxR;
        p->chunks.push_back(ch);
    }
    const size_t n_list = l64.size() + l16.size() + 2 * gen.size();
    if (n_list > 0) {
        const size_t o16 = align16(l64.size() * 4), og = o16 + align16(l16.size() * 4), ob = og + align16(gen.size() * 4);
        const size_t lb = ob + align16(gen.size() * 4);
        if (p->lists.alloc(p->dev, lb) != hipSuccess) return SBLAS_E_HIP;
        p->bytes += lb;
        p->list64 = p->lists.at<int32_t>(), p->list16 = p->lists.at<int32_t>(o16);
        p->gen_rows = p->lists.at<int32_t>(og), p->gen_abase = p->lists.at<int32_t>(ob);
        e = hipSuccess;
        if (!l64.empty()) e = hipMemcpyAsync(p->list64, l64.data(), l64.size() * 4, hipMemcpyHostToDevice, s);
        if (e == hipSuccess && !l16.empty()) e = hipMemcpyAsync(p->list16, l16.data(), l16.size() * 4, hipMemcpyHostToDevice, s);
        if (e == hipSuccess && !gen.empty()) e = hipMemcpyAsync(p->gen_rows, gen.data(), gen.size() * 4, hipMemcpyHostToDevice, s);
        if (e == hipSuccess && !gen.empty()) e = hipMemcpyAsync(p->gen_abase, gen_abase.data(), gen.size() * 4, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s); // the host vectors are read until here
        if (e != hipSuccess) return SBLAS_E_HIP;
    }
    if (n_chunks > 0) {
        const size_t wb = gen_layout(maxP, maxNA, maxR, nullptr, nullptr);
        if (p->work.alloc(p->dev, wb) != hipSuccess) return SBLAS_E_HIP;
        gen_layout(maxP, maxNA, maxR, p->work.at<char>(), &p->gw);
        p->bytes += wb;
    }

    // symbolic: the rows' counts, their sum as a 64-bit integer, the scan, then the columns
    unsigned long long total = 0;
    if (m > 0) {
        uint32_t *counts = reinterpret_cast<uint32_t *>(p->rowptr_c);
        unsigned long long *d_total = small.at<unsigned long long>(8);
        e = hipMemsetAsync(d_total, 0, 8, s);
        if (e == hipSuccess) e = launch_symbolic<false>(*p, s, counts);
        if (e == hipSuccess) {
            sum_counts_kernel<<<grid_for(m), T_THREADS, 0, s>>>(m, counts, d_total);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return SBLAS_E_HIP;
        if (sblas_hip_spgemm_check_nnz((int64_t)total) != SBLAS_OK) return SBLAS_E_INVALID;
        const int64_t nb = ceil_div(m + 1, SCAN_TILE);
        DeviceBuffer bsum;
        if (bsum.alloc(p->dev, align16((size_t)nb * 4)) != hipSuccess) return SBLAS_E_HIP;
        e = scan_exclusive(s, counts, m + 1, bsum.at<uint32_t>(), nb);
        if (e == hipSuccess) e = hipStreamSynchronize(s); // bsum is freed here
        if (e != hipSuccess) return SBLAS_E_HIP;
    }
    p->nnz_c = (int64_t)total;
    if (p->nnz_c > 0) {
        const size_t cc = align16((size_t)p->nnz_c * 4);
        if (p->colidx_buf.alloc(p->dev, cc) != hipSuccess) return SBLAS_E_HIP;
        p->colidx_c = p->colidx_buf.at<int32_t>();
        p->bytes += cc;
        e = launch_symbolic<true>(*p, s, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return SBLAS_E_HIP;
    }
    *plan_out = p.release();
    return SBLAS_OK;
}

int sblas_hip_spgemm_plan_info(const void *plan, int64_t out[12])
{
    if (!plan || !out) return SBLAS_E_INVALID;
    const SpgemmPlan *p = static_cast<const SpgemmPlan *>(plan);
    out[0] = p->m, out[1] = p->k, out[2] = p->n, out[3] = p->nnz_c, out[4] = p->products, out[5] = p->rows64 + p->rows16;
    out[6] = p->rows_general, out[7] = (int64_t)p->chunks.size(), out[8] = p->max_row_products, out[9] = p->b_ascending;
    out[10] = (int64_t)p->bytes, out[11] = p->flags;
    return SBLAS_OK;
}

int sblas_hip_spgemm_plan_csr(const void *plan, const int32_t **rowptr_c, const int32_t **colidx_c)
{
    if (!plan) return SBLAS_E_INVALID;
    const SpgemmPlan *p = static_cast<const SpgemmPlan *>(plan);
    if (rowptr_c) *rowptr_c = p->rowptr_c;
    if (colidx_c) *colidx_c = p->colidx_c;
    return SBLAS_OK;
}

int sblas_hip_spgemm_plan_numeric(const void *plan, void *stream, const double *val_a, const double *val_b, double *val_c)
{
    if (!plan) return SBLAS_E_INVALID;
    const SpgemmPlan *p = static_cast<const SpgemmPlan *>(plan);
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID; // the plan's arrays live on its own device
    if (p->nnz_c == 0) return SBLAS_OK;
    if (!val_a || !val_b || !val_c) return SBLAS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (p->rows64 > 0)
        row_numeric_kernel<64><<<row_grid(p->rows64, 1), 64, 0, s>>>(p->rows64, p->list64, p->rowptr_a, p->colidx_a, val_a, p->rowptr_b,
                                                                    p->colidx_b, val_b, p->rowptr_c, p->colidx_c, val_c);
    if (p->rows16 > 0)
        row_numeric_kernel<sblas::SPGEMM_NARROW><<<row_grid(p->rows16, 64 / sblas::SPGEMM_NARROW), 64, 0, s>>>(
            p->rows16, p->list16, p->rowptr_a, p->colidx_a, val_a, p->rowptr_b, p->colidx_b, val_b, p->rowptr_c, p->colidx_c, val_c);
    hipError_t e = hipGetLastError();
    for (size_t c = 0; c < p->chunks.size() && e == hipSuccess; ++c) {
        const Chunk &ch = p->chunks[c];
        e = run_chunk(*p, s, ch, val_a, val_b);
        if (e != hipSuccess) break;
        gen_place_kernel<double><<<sg_grid(ch.R), T_THREADS, 0, s>>>(ch.R, p->gen_rows + ch.g0, p->gw.rowptr_loc, p->gw.val_loc, p->rowptr_c, val_c);
        e = hipGetLastError();
    }
    return e == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_spgemm_plan_destroy(void *plan)
{
    delete static_cast<SpgemmPlan *>(plan);
    return SBLAS_OK;
}

} // extern "C"
