// coo_sum.h -- the sorted, run-summed CSR of a set of triplets, as coo.hip's entry points and spgemm.hip's general path
// both compute it: the workspace layout, the structure kernels, the run-sum kernel and run_coo, which strings them onto
// a stream.  coo.hip's header comment describes the passes and the order.  Internal to each translation unit: nothing
// here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sblas_hip.h"
#include "radix_sort.h"

namespace {

constexpr int SUM_CHUNK = 2048; // sorted positions per LDS chunk of the sum kernel (16 KiB)

struct CooWorkspace {
    Workspace sort;            // keys / payload ping-pong (nnz + 1 entries each), digit counts, block sums
    int64_t mark_blocks = 0;   // scan blocks of the nnz + 1 head marks (they share sort.bsum)
};

// four int32 arrays of nnz + 1 entries (16 B per triplet), 1 KiB of digit counts per 4096 triplets and the block sums of
// the larger of the two scans (the digit counts', the head marks')
inline size_t coo_layout(int64_t nnz, char *base, CooWorkspace *w)
{
    const int64_t tiles = ceil_div(nnz, T_TILE), hist_len = (int64_t)RADIX * tiles, scan_blocks = ceil_div(hist_len, SCAN_TILE);
    const int64_t mark_blocks = ceil_div(nnz + 1, SCAN_TILE);
    const size_t arr = align16(((size_t)nnz + 1) * sizeof(int32_t)), hist = align16((size_t)hist_len * sizeof(uint32_t));
    const size_t bsum = align16((size_t)(scan_blocks > mark_blocks ? scan_blocks : mark_blocks) * sizeof(uint32_t));
    if (w) {
        Workspace &s = w->sort;
        s.tiles = tiles, s.hist_len = hist_len, s.scan_blocks = scan_blocks, w->mark_blocks = mark_blocks;
        size_t off = 0;
        for (int q = 0; q < 2; ++q) {
            s.keys[q] = reinterpret_cast<int32_t *>(base + off), off += arr;
            s.idx[q] = reinterpret_cast<int32_t *>(base + off), off += arr;
        }
        s.hist = reinterpret_cast<uint32_t *>(base + off), off += hist;
        s.bsum = reinterpret_cast<uint32_t *>(base + off);
    }
    return 4 * arr + hist + bsum;
}

// dst[i] = src[idx[i]]: the row keys in the column-sorted order
__global__ __launch_bounds__(T_THREADS) void gather_i32_kernel(int64_t n, const int32_t *__restrict__ idx,
                                                               const int32_t *__restrict__ src, int32_t *__restrict__ dst)
{
    for (int64_t i = (int64_t)blockIdx.x * T_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * T_THREADS) dst[i] = src[idx[i]];
}

// KEEP: position i holds triplet k = sidx[i] (identity when no pass ran).  Thread 0 closes runptr (also for nnz == 0).
__global__ __launch_bounds__(T_THREADS) void coo_keep_finish_kernel(const int32_t *__restrict__ sidx, int64_t nnz,
                                                                    const int32_t *__restrict__ coo_col,
                                                                    const double *__restrict__ coo_val, int32_t *__restrict__ colidx,
                                                                    double *__restrict__ val, int32_t *__restrict__ perm,
                                                                    int32_t *__restrict__ runptr)
{
    const int64_t t0 = (int64_t)blockIdx.x * T_THREADS + threadIdx.x;
    if (t0 == 0 && runptr) runptr[nnz] = (int32_t)nnz;
    for (int64_t i = t0; i < nnz; i += (int64_t)gridDim.x * T_THREADS) {
        const int32_t k = sidx ? sidx[i] : (int32_t)i;
        colidx[i] = coo_col[k];
        if (val) val[i] = coo_val[k];
        if (perm) perm[i] = k;
        if (runptr) runptr[i] = (int32_t)i;
    }
}

// SUM: the sorted columns and marks[i] = 1 where a run starts; marks[nnz] = 0.  A lane takes the column of position
// i - 1 from the lane below it; only a wave's first lane gathers it again.
__global__ __launch_bounds__(T_THREADS) void coo_heads_kernel(const int32_t *__restrict__ skeys, const int32_t *__restrict__ sidx,
                                                              int64_t nnz, const int32_t *__restrict__ coo_col,
                                                              int32_t *__restrict__ scol, uint32_t *__restrict__ marks,
                                                              int32_t *__restrict__ perm)
{
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * T_THREADS; base <= nnz; base += (int64_t)gridDim.x * T_THREADS) {
        const int64_t i = base + threadIdx.x;
        const bool valid = i < nnz;
        const int32_t k = valid ? (sidx ? sidx[i] : (int32_t)i) : 0;
        const int32_t c = valid ? coo_col[k] : 0;
        int32_t before = __shfl_up(c, 1, 64);
        if (valid) {
            if (lane == 0 && i > 0) before = coo_col[sidx ? sidx[i - 1] : (int32_t)(i - 1)];
            scol[i] = c;
            marks[i] = (i == 0 || skeys[i] != skeys[i - 1] || c != before) ? 1u : 0u;
            if (perm) perm[i] = k;
        } else if (i == nnz) {
            marks[i] = 0u;
        }
    }
}

// SUM: position i starts entry before[i] when the count moves on behind it
__global__ __launch_bounds__(T_THREADS) void coo_compact_kernel(const uint32_t *__restrict__ before, int64_t nnz,
                                                                const int32_t *__restrict__ scol, int32_t *__restrict__ colidx,
                                                                int32_t *__restrict__ runptr)
{
    const int64_t t0 = (int64_t)blockIdx.x * T_THREADS + threadIdx.x;
    if (t0 == 0) runptr[before[nnz]] = (int32_t)nnz;
    for (int64_t i = t0; i < nnz; i += (int64_t)gridDim.x * T_THREADS) {
        const uint32_t e = before[i];
        if (before[i + 1] != e) {
            colidx[e] = scol[i];
            runptr[e] = (int32_t)i;
        }
    }
}

// val_out[e] = the left-to-right sum of coo_val[perm[k]], k in [runptr[e], runptr[e + 1]); *count entries.  perm ==
// nullptr is the identity.  A run of one is copied (no add: -0.0 stays -0.0).
__global__ __launch_bounds__(T_THREADS) void coo_assemble_sum_kernel(const int32_t *__restrict__ count,
                                                                     const int32_t *__restrict__ runptr,
                                                                     const int32_t *__restrict__ perm,
                                                                     const double *__restrict__ coo_val, double *__restrict__ val_out)
{
    __shared__ double buf[SUM_CHUNK];
    const int64_t entries = *count;
    const int tid = threadIdx.x;
    for (int64_t e0 = (int64_t)blockIdx.x * T_THREADS; e0 < entries; e0 += (int64_t)gridDim.x * T_THREADS) {
        const int64_t e = e0 + tid, e1 = e0 + T_THREADS < entries ? e0 + T_THREADS : entries;
        const bool live = e < entries;
        const int64_t s = live ? runptr[e] : 0, t = live ? runptr[e + 1] : 0;
        const int64_t p0 = runptr[e0], p1 = runptr[e1]; // the workgroup's positions
        double acc = 0.0;
        for (int64_t c0 = p0; c0 < p1; c0 += SUM_CHUNK) {
            const int64_t c1 = c0 + SUM_CHUNK < p1 ? c0 + SUM_CHUNK : p1;
            __syncthreads(); // the chunk before has been added
            for (int64_t p = c0 + tid; p < c1; p += T_THREADS) buf[p - c0] = coo_val[perm ? perm[p] : (int32_t)p];
            __syncthreads();
            const int64_t lo = s > c0 ? s : c0, hi = t < c1 ? t : c1;
            for (int64_t k = lo; k < hi; ++k) {
                const double v = buf[k - c0];
                acc = k == s ? v : acc + v;
            }
        }
        if (live) val_out[e] = acc;
    }
}

hipError_t run_coo(hipStream_t s, int64_t rows, int64_t cols, int64_t nnz, const int32_t *coo_row, const int32_t *coo_col,
                   const double *coo_val, int dup, int32_t *rowptr, int32_t *colidx, double *val, int32_t *perm, int32_t *runptr,
                   void *workspace)
{
    if (nnz == 0) { // every row is empty; runptr = {0}
        colptr_kernel<<<grid_for(rows + 1), T_THREADS, 0, s>>>(nullptr, 0, rows, nullptr, rowptr);
        if (runptr) coo_keep_finish_kernel<<<1, T_THREADS, 0, s>>>(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, runptr);
        return hipGetLastError();
    }
    CooWorkspace w;
    coo_layout(nnz, static_cast<char *>(workspace), &w);
    const int cpasses = radix_passes(cols), rpasses = radix_passes(rows), passes = cpasses + rpasses;
    const int32_t *skeys = coo_col, *sidx = nullptr;
    int p = 0;
    for (; p < cpasses; ++p) {
        const hipError_t e = radix_pass(s, w.sort, skeys, sidx, nnz, p * RADIX_BITS, p & 1);
        if (e != hipSuccess) return e;
        skeys = w.sort.keys[p & 1], sidx = w.sort.idx[p & 1];
    }
    if (cpasses > 0) { // the row keys in the column-sorted order take the place of the sorted column keys
        int32_t *rkeys = w.sort.keys[(cpasses - 1) & 1];
        gather_i32_kernel<<<grid_for(nnz), T_THREADS, 0, s>>>(nnz, sidx, coo_row, rkeys);
        skeys = rkeys;
    } else {
        skeys = coo_row;
    }
    for (int r = 0; r < rpasses; ++r, ++p) {
        const hipError_t e = radix_pass(s, w.sort, skeys, sidx, nnz, r * RADIX_BITS, p & 1);
        if (e != hipSuccess) return e;
        skeys = w.sort.keys[p & 1], sidx = w.sort.idx[p & 1];
    }
    if (dup == SBLAS_COO_KEEP) {
        colptr_kernel<<<grid_for(rows + 1), T_THREADS, 0, s>>>(skeys, nnz, rows, nullptr, rowptr);
        coo_keep_finish_kernel<<<grid_for(nnz), T_THREADS, 0, s>>>(sidx, nnz, coo_col, coo_val, colidx, val, perm, runptr);
        return hipGetLastError();
    }
    // the pair of buffers the last pass did not write is free; so is the sorted row keys' once rowptr is made
    const int spare = passes & 1, last = passes > 0 ? (passes - 1) & 1 : 1;
    int32_t *scol = w.sort.keys[spare];
    uint32_t *marks = reinterpret_cast<uint32_t *>(w.sort.idx[spare]);
    int32_t *runs = runptr ? runptr : w.sort.keys[last];
    coo_heads_kernel<<<grid_for(nnz + 1), T_THREADS, 0, s>>>(skeys, sidx, nnz, coo_col, scol, marks, perm);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = scan_exclusive(s, marks, nnz + 1, w.sort.bsum, w.mark_blocks);
    if (e != hipSuccess) return e;
    colptr_kernel<<<grid_for(rows + 1), T_THREADS, 0, s>>>(skeys, nnz, rows, marks, rowptr);
    coo_compact_kernel<<<grid_for(nnz), T_THREADS, 0, s>>>(marks, nnz, scol, colidx, runs);
    if (val) coo_assemble_sum_kernel<<<grid_for(nnz), T_THREADS, 0, s>>>(rowptr + rows, runs, sidx, coo_val, val);
    return hipGetLastError();
}

} // namespace
