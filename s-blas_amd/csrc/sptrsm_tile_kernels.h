// sptrsm_tile_kernels.h -- sptrsv.hip's SpSV kernels widened by a tile of SPTRSM_TILE columns:
// T X = alpha B on n x s row-major blocks.  Included by sptrsv.hip alone, after its Unit, finish_row() and solve_row(),
// whose text this file restates column by column:
//   solve_row_tile   solve_row over a tile: the same G(p) lanes from the stored length, lane l the entries l, l + G, ...
//                    in stored order; a lane fetches colidx[e] ONCE per entry, applies the triangle predicate once, and
//                    for a selected entry fetches val[e] once and then the eight doubles X[c * ldx + j0 .. j0 + 7]; eight
//                    accumulators from +0 with one fused multiply-add each, eight butterflies; the writer lane loads the
//                    pivot once and its eight b ahead of the fold, applies finish_row to each column and stores eight
//                    doubles.
// An entry outside the triangle is SKIPPED, never multiplied by zero: neither its value nor X at its column is loaded, so
// a NaN or an Inf stored in the ignored triangle stays invisible.  Column c of a tile goes through exactly the operations
// of solve_row in the same order, so column j of X has the single solve's bits on column j of B; no column's value enters
// another column's arithmetic.
//
// Width of the accesses.  FAST: a full tile whose launch has both bases and both leading dimensions a multiple of 16
// bytes (decided on the host) moves a row's eight doubles as four 16-byte accesses.  Anything else -- the ragged last
// tile, an odd leading dimension, a base offset by one element -- goes double by double under the column mask; a column
// outside the mask is neither read nor written.  Same values, same order, same bits.
//
// X and B carry no __restrict__: they may be the same block (in place, with equal leading dimensions).  Only row i's
// writer lane reads b[i, tile], and it does so before it stores x[i, tile].
//
// The chain kernel runs one workgroup PER TILE.  Each walks the whole run of levels for its own eight columns with
// __syncthreads() between levels, as the single chain kernel does; why a workgroup sees what it needs with other
// workgroups writing next to it is argued in DESIGN.md 3.31.  No LDS, no atomics, nothing waits across workgroups.
#pragma once
#include <type_traits>
#include "sptrsm_tile.h"

namespace {

constexpr int ST = SPTRSM_TILE;

template <bool FAST> __device__ __forceinline__ void sptrsm_ld8(const double *p, unsigned mask, double (&x)[ST])
{
    if constexpr (FAST) {
        const double2 *q = reinterpret_cast<const double2 *>(p);
#pragma unroll
        for (int c = 0; c < ST / 2; ++c) {
            const double2 t = q[c];
            x[2 * c] = t.x, x[2 * c + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int c = 0; c < ST; ++c) x[c] = (mask >> c & 1u) ? p[c] : 0.0;
    }
}

template <bool FAST> __device__ __forceinline__ void sptrsm_st8(double *p, unsigned mask, const double (&x)[ST])
{
    if constexpr (FAST) {
        double2 *q = reinterpret_cast<double2 *>(p);
#pragma unroll
        for (int c = 0; c < ST / 2; ++c) q[c] = make_double2(x[2 * c], x[2 * c + 1]);
    } else {
#pragma unroll
        for (int c = 0; c < ST; ++c)
            if (mask >> c & 1u) p[c] = x[c];
    }
}

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
    double bi[ST], s[ST];
#pragma unroll
    for (int c = 0; c < ST; ++c) bi[c] = s[c] = 0.0;
    if (writer) sptrsm_ld8<FAST>(b + (int64_t)u.row * a.ldb, mask, bi); // read before x[row, tile] is written: in place is fine
    if (u.row >= 0) {
        for (int64_t e = (int64_t)u.beg + lane; e < u.end; e += G) {
            const int c = colidx[e];
            if (lower ? c < u.row : c > u.row) { // the other triangle is never loaded: not its value, not X at its column
                const double v = val[e];
                double xv[ST];
                sptrsm_ld8<FAST>(x + (int64_t)c * a.ldx, mask, xv);
#pragma unroll
                for (int k = 0; k < ST; ++k) s[k] = __builtin_fma(v, xv[k], s[k]);
            }
        }
    }
    double f[ST];
#pragma unroll
    for (int k = 0; k < ST; ++k) {
        const double f4 = fold_sum<4>(s[k]);
        double f16 = f4 + lane_partner<4>(f4);
        f16 += lane_partner<8>(f16);
        double f64 = f16 + lane_partner<16>(f16);
        f64 += lane_partner<32>(f64);
        f[k] = gs == 2 ? f4 : gs == 4 ? f16 : f64;
    }
    if (writer) {
        double out[ST];
#pragma unroll
        for (int k = 0; k < ST; ++k) out[k] = finish_row(a.alpha, bi[k], f[k], pivot);
        sptrsm_st8<FAST>(x + (int64_t)u.row * a.ldx, mask, out);
    }
}

// Which unit block and which column tile a workgroup of a wide launch takes: the numbering of amg_multi_kernels.h, which
// keeps a unit block's tiles SPTRSM_GROUP ids apart.  It cannot reach a bit: a (unit, tile) pair computes the same sums
// wherever it runs.
struct SptrsmTileId {
    int64_t block, tile;
};
__device__ __forceinline__ SptrsmTileId sptrsm_tile_id(int64_t blocks, int64_t tiles)
{
    const int64_t per = SPTRSM_GROUP * tiles, id = blockIdx.x, g = id / per, rem = id - g * per;
    const int64_t left = blocks - SPTRSM_GROUP * g, gb = left < SPTRSM_GROUP ? left : SPTRSM_GROUP; // the last group is short
    return SptrsmTileId{SPTRSM_GROUP * g + rem % gb, rem / gb};
}

// ---- wide: one level, (the level's unit blocks) x tiles workgroups; wide_unit()'s layout with the unit block given
// instead of read off blockIdx.x
template <bool WIDE>
__global__ __launch_bounds__(SPTRSM_WIDE_THREADS) void sptrsm_tile_wide_kernel(int64_t first, int64_t count, int64_t blocks, const TileSolveArgs a)
{
    const int64_t tiles = sptrsm_tiles(a.s);
    const SptrsmTileId id = sptrsm_tile_id(blocks, tiles);
    const int64_t j0 = id.tile * ST, w = a.s - j0 < ST ? a.s - j0 : ST;
    const unsigned mask = (1u << w) - 1u;
    const int64_t k = (id.block * SPTRSM_WIDE_THREADS + threadIdx.x) >> 2;
    const Unit u = k < count ? load_unit(a.units, first + k) : NO_UNIT;
    if (WIDE && w == ST) solve_row_tile<true>(u, threadIdx.x & 3, a, a.b + j0, a.x + j0, mask);
    else solve_row_tile<false>(u, threadIdx.x & 3, a, a.b + j0, a.x + j0, mask);
}

// ---- chain: levels l0 .. l1 - 1, one workgroup a tile; chain_walk unchanged, the tile row as its callable
template <bool WIDE>
__global__ __launch_bounds__(SPTRSV_CHAIN_THREADS) void sptrsm_tile_chain_kernel(int64_t l0, int64_t l1, const int64_t *__restrict__ level_unit_ptr,
                                                                                 const TileSolveArgs a)
{
    const int64_t j0 = (int64_t)blockIdx.x * ST, w = a.s - j0 < ST ? a.s - j0 : ST;
    const unsigned mask = (1u << w) - 1u;
    const double *b = a.b + j0;
    double *x = a.x + j0;
    if (WIDE && w == ST)
        chain_walk<SPTRSV_CHAIN_THREADS>(l0, l1, level_unit_ptr, a.units, NO_UNIT,
                                         [&](const Unit u) { solve_row_tile<true>(u, threadIdx.x & 3, a, b, x, mask); });
    else
        chain_walk<SPTRSV_CHAIN_THREADS>(l0, l1, level_unit_ptr, a.units, NO_UNIT,
                                         [&](const Unit u) { solve_row_tile<false>(u, threadIdx.x & 3, a, b, x, mask); });
}

// ---- launches ----------------------------------------------------------------------------------------------------------
inline bool sptrsm_wide16(const void *p, int64_t ld) { return ((reinterpret_cast<uintptr_t>(p) | (uintptr_t)(ld * 8)) & 15u) == 0; }

} // namespace
