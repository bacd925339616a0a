// sptrsm_tile_kernels.h -- the two kernels of the tiled SpSM: T X = alpha B on n x s row-major blocks.
// Included by sptrsv.hip alone, after its Unit, finish_row() and solve_row().  solve_row_tile is solve_row's loop eight
// columns abreast, kept as its own text over the shared tile_ld / tile_st, group_fold and tile_id (unit_row.h; why not
// one text: DESIGN.md 3.32): the same G(p) lanes from the stored length, lane l the entries l, l + G, ... in stored
// order; a lane fetches colidx[e] once per entry, applies the triangle predicate once, and for a selected entry fetches
// val[e] once and then the eight doubles X[c * ldx + j0 .. j0 + 7]; eight accumulators from +0 with one fused
// multiply-add each, eight folds; the writer lane applies finish_row to each column.  An entry outside the triangle is
// SKIPPED, never multiplied by zero.  Column c of a tile goes through exactly the operations of solve_row in the same
// order, so column j of X has the single solve's bits on column j of B.
//
// The grid.  A wide launch is (the level's unit blocks) x tiles workgroups, numbered by tile_id(); FAST is taken by a
// full tile of a launch whose bases and leading dimensions are multiples of 16 bytes (wide16(), decided on the host).
//
// X and B carry no __restrict__: they may be the same block (in place, with equal leading dimensions).  Only row i's
// writer lane reads b[i, tile], and it does so before it stores x[i, tile].
//
// The chain kernel runs one workgroup PER TILE.  Each walks the whole run of levels for its own eight columns with
// __syncthreads() between levels, as the single chain kernel does; why a workgroup sees what it needs with other
// workgroups writing next to it is argued in DESIGN.md 3.31.  No LDS, no atomics, nothing waits across workgroups.
#pragma once
#include "sptrsm_tile.h"

namespace {

// what a launch of either kernel reads: b and x are the blocks' bases, the tile's first column is added by the kernel
struct TileSolveArgs {
    int lower;
    int64_t s; // columns
    const Unit *units;
    const int32_t *colidx;
    const double *val;
    double alpha;
    const double *b;
    int64_t ldb;
    double *x;
    int64_t ldx;
};

// X[row, j0 .. j0 + 7] for the row of unit u; b and x point at column j0.  Every lane of the wave calls this together
// (the butterflies move data between lanes); `quad` is the lane's place in its unit.
template <bool FAST>
__device__ __forceinline__ void solve_row_tile(const Unit u, int quad, const TileSolveArgs &a, const double *b, double *x, unsigned mask)
{
    const bool lower = a.lower != 0;
    const int32_t *__restrict__ colidx = a.colidx;
    const double *__restrict__ val = a.val;
    const int gs = sptrsv_group_shift((int64_t)u.end - u.beg), G = 1 << gs;
    const int lane = (u.tag <= -2 ? 4 * (-2 - u.tag) : 0) + quad; // the lane's place among the row's G lanes
    const bool writer = u.row >= 0 && lane == 0;
    // the row's pivot and right-hand sides travel with its first entries instead of waiting behind the fold
    const double pivot = writer && u.tag >= 0 ? val[u.tag] : 1.0;
    double bi[TILE], s[TILE];
#pragma unroll
    for (int c = 0; c < TILE; ++c) bi[c] = s[c] = 0.0;
    if (writer) tile_ld<TILE, FAST>(b + (int64_t)u.row * a.ldb, mask, bi); // read before x[row, tile] is written: in place is fine
    if (u.row >= 0) {
        for (int64_t e = (int64_t)u.beg + lane; e < u.end; e += G) {
            const int c = colidx[e];
            if (lower ? c < u.row : c > u.row) { // the other triangle is never loaded: not its value, not X at its column
                const double v = val[e];
                double xv[TILE];
                tile_ld<TILE, FAST>(x + (int64_t)c * a.ldx, mask, xv);
#pragma unroll
                for (int k = 0; k < TILE; ++k) s[k] = __builtin_fma(v, xv[k], s[k]);
            }
        }
    }
    double f[TILE];
#pragma unroll
    for (int k = 0; k < TILE; ++k) f[k] = group_fold(s[k], gs);
    if (writer) {
        double out[TILE];
#pragma unroll
        for (int k = 0; k < TILE; ++k) out[k] = finish_row(a.alpha, bi[k], f[k], pivot);
        tile_st<TILE, FAST>(x + (int64_t)u.row * a.ldx, mask, out);
    }
}

// ---- wide: one level, (the level's unit blocks) x tiles workgroups; wide_unit()'s layout with the unit block given
// instead of read off blockIdx.x
template <bool WIDE>
__global__ __launch_bounds__(SPTRSM_WIDE_THREADS) void sptrsm_tile_wide_kernel(int64_t first, int64_t count, int64_t blocks, const TileSolveArgs a)
{
    const TileId id = tile_id(blocks, tiles(a.s));
    const int64_t j0 = id.tile * TILE, w = a.s - j0 < TILE ? a.s - j0 : TILE;
    const unsigned mask = (1u << w) - 1u;
    const int64_t k = (id.block * SPTRSM_WIDE_THREADS + threadIdx.x) >> 2;
    const Unit u = k < count ? load_unit(a.units, first + k) : NO_UNIT;
    if (WIDE && w == TILE) solve_row_tile<true>(u, threadIdx.x & 3, a, a.b + j0, a.x + j0, mask);
    else solve_row_tile<false>(u, threadIdx.x & 3, a, a.b + j0, a.x + j0, mask);
}

// ---- chain: levels l0 .. l1 - 1, one workgroup a tile; chain_walk unchanged, the tile row as its callable
template <bool WIDE>
__global__ __launch_bounds__(SPTRSV_CHAIN_THREADS) void sptrsm_tile_chain_kernel(int64_t l0, int64_t l1, const int64_t *__restrict__ level_unit_ptr,
                                                                                 const TileSolveArgs a)
{
    const int64_t j0 = (int64_t)blockIdx.x * TILE, w = a.s - j0 < TILE ? a.s - j0 : TILE;
    const unsigned mask = (1u << w) - 1u;
    const double *b = a.b + j0;
    double *x = a.x + j0;
    if (WIDE && w == TILE)
        chain_walk<SPTRSV_CHAIN_THREADS>(l0, l1, level_unit_ptr, a.units, NO_UNIT, [&](const Unit u) { solve_row_tile<true>(u, threadIdx.x & 3, a, b, x, mask); });
    else
        chain_walk<SPTRSV_CHAIN_THREADS>(l0, l1, level_unit_ptr, a.units, NO_UNIT, [&](const Unit u) { solve_row_tile<false>(u, threadIdx.x & 3, a, b, x, mask); });
}

} // namespace
