// krylov_tile.h -- a cell's walk and the store of a tile's lane sums, shared by the widened solver kernels
// (krylov_multi.hip, gmres_multi.hip): a workgroup is a cell of KRYLOV_CELL rows and a tile of TILE columns (tile.h).
// Additions only, so nothing here can be contracted; the files that include it switch contraction off for the products
// they feed in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "krylov.h"
#include "krylov_fold.h"
#include "tile.h"

namespace sblas {

// Lane t of a cell takes rows t, t + 256, ... of the cell in that order (cell_walk's order); absent rows are skipped.
// Not unrolled eight times as cell_walk is: a row is already eight columns of every operand in registers.
template <class F> __device__ __forceinline__ void row_walk(int64_t cell, int64_t n, F f)
{
    const int64_t first = cell * KRYLOV_CELL;
#pragma unroll 2
    for (int k = 0; k < KRYLOV_PER_LANE; ++k) {
        const int64_t i = first + threadIdx.x + k * KRYLOV_LANES;
        if (i < n) f(i);
    }
}

// the tile's ND * TILE lane sums through group_fold; lane 0 stores the columns of the mask
template <int ND>
__device__ __forceinline__ void tile_store(const double (&acc)[ND * TILE], double *part, int s, int64_t cells, int64_t cell, int j0, unsigned mask)
{
    double out[ND * TILE];
    group_fold<ND * TILE>(acc, out);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < ND; ++k)
#pragma unroll
            for (int c = 0; c < TILE; ++c)
                if (mask >> c & 1u) part[((int64_t)k * s + j0 + c) * cells + cell] = out[k * TILE + c];
    }
}

} // namespace sblas
