// krylov_fold.h -- the device helpers that pin a dot product's order, shared by krylov.hip and gmres.hip: a cell's walk,
// the butterfly inside a wave and the fold of a workgroup's four waves.  Additions only, so nothing here can be
// contracted; the files that include it switch contraction off for the products they feed in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "krylov.h"

namespace sblas {

// the butterfly l ^ 1 .. l ^ 32 inside a wave: every lane ends with the same bits (IEEE addition commutes)
__device__ __forceinline__ double wave_fold(double v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m);
    return v;
}

// The 256 lane sums of NP dots folded by the butterfly l ^ 1 .. l ^ 128; steps 64 and 128 go through LDS: lane 0 of the
// butterfly ends with (w0 + w1) + (w2 + w3) of the four waves' sums.  Every thread returns with out[] set.
template <int NP> __device__ __forceinline__ void group_fold(const double (&acc)[NP], double (&out)[NP])
{
    __shared__ double ws[NP][4];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const double v = wave_fold(acc[q]);
        if ((threadIdx.x & 63) == 0) ws[q][threadIdx.x >> 6] = v;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NP; ++q) out[q] = (ws[q][0] + ws[q][1]) + (ws[q][2] + ws[q][3]);
}

// Stage 2 of nd <= KRYLOV_MAX_DOTS dots: lane t adds partial[t], partial[t + 256], ... of each dot in order from +0, then
// the same butterfly.  Dot q's cells' sums start at part + q * stride.  Every thread returns with d[] set.
__device__ __forceinline__ void cells_fold(int nd, int64_t cells, const double *part, int64_t stride, double (&d)[KRYLOV_MAX_DOTS])
{
    double acc[KRYLOV_MAX_DOTS] = {};
    for (int64_t c = threadIdx.x; c < cells; c += KRYLOV_LANES)
        for (int q = 0; q < nd; ++q) acc[q] = acc[q] + part[q * stride + c];
    group_fold<KRYLOV_MAX_DOTS>(acc, d);
}

// Lane t of cell c takes elements t, t + 256, ... of the cell in that order; absent elements are skipped.
template <class F> __device__ __forceinline__ void cell_walk(int64_t n, F f)
{
    const int64_t first = (int64_t)blockIdx.x * KRYLOV_CELL;
    if (first + KRYLOV_CELL <= n) {
#pragma unroll
        for (int k = 0; k < KRYLOV_PER_LANE; ++k) f(first + threadIdx.x + k * KRYLOV_LANES);
    } else {
        for (int k = 0; k < KRYLOV_PER_LANE; ++k) {
            const int64_t i = first + threadIdx.x + k * KRYLOV_LANES;
            if (i < n) f(i);
        }
    }
}

template <int NP> __device__ __forceinline__ void cell_store(const double (&acc)[NP], double *part, int64_t cells)
{
    double out[NP];
    group_fold<NP>(acc, out);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < NP; ++q) part[q * cells + blockIdx.x] = out[q];
    }
}

} // namespace sblas
