// amg_multi_kernels.h -- the kernels of the block cycle Z = M^-1 R on n x s row-major blocks.  Included
// by amg.hip alone, after its modes and its single-column kernels:
//   sweep / residual   sweep_row's loop eight columns abreast, kept as its own text over the shared tile_ld / tile_st,
//                      group_fold and tile_id (unit_row.h; why not one text: DESIGN.md 3.32): a lane fetches val[e] and
//                      colidx[e] ONCE per entry and then the eight doubles X[col * ldx + j0 .. j0 + 7]; eight
//                      accumulators, eight folds; the writer lane reads b, x, wd for its row and tile and stores eight
//                      doubles;
//   transfer           transfer_row the same way (a smoothed plan's R_l and P_l);
//   first, restrict, prolong   one thread per (row or aggregate, column), columns fastest.
// Column c of a tile goes through exactly the operations of the single kernel in the same order -- one fused
// multiply-add per entry from +0 in the lane order of G(p), group_fold, then the row's last step rounded operation by
// operation (contraction is off at amg.hip's file scope, ahead of this include) -- so column j of a block has the single
// kernel's bits on that column.  No column's value enters another column's arithmetic.
//
// The grid of a row kernel is (unit blocks) x tiles workgroups, numbered by tile_id(); FAST is taken by a full tile of a
// launch whose every base and leading dimension is a multiple of 16 bytes (wide16(), decided on the host).
//
// No LDS, no atomics, nothing waits across workgroups.
#pragma once
#include "amg_multi.h"

namespace {

// wide_unit() with the unit block given instead of read off blockIdx.x
__device__ __forceinline__ SweepUnit multi_unit(int64_t block, int64_t count, const SweepUnit *__restrict__ units)
{
    const int64_t u = (block * AMG_THREADS + threadIdx.x) >> 2;
    return u < count ? load_unit(units, u) : NO_SWEEP_UNIT;
}

// the row sums of a tile: sweep_row's loop and fold, eight columns abreast; the writer lane's f[c] is column c's sum
template <bool FAST>
__device__ __forceinline__ void tile_row_sums(const SweepUnit u, int gs, int lane, const int32_t *__restrict__ colidx, const double *__restrict__ val,
                                              const double *__restrict__ x, int64_t ldx, unsigned mask, double (&f)[TILE])
{
    const int G = 1 << gs;
    double s[TILE];
#pragma unroll
    for (int c = 0; c < TILE; ++c) s[c] = 0.0;
    if (u.row >= 0)
        for (int64_t e = (int64_t)u.beg + lane; e < u.end; e += G) {
            const double a = val[e];
            double xv[TILE];
            tile_ld<TILE, FAST>(x + (int64_t)colidx[e] * ldx, mask, xv);
#pragma unroll
            for (int c = 0; c < TILE; ++c) s[c] = __builtin_fma(a, xv[c], s[c]);
        }
#pragma unroll
    for (int c = 0; c < TILE; ++c) f[c] = group_fold(s[c], gs);
}

struct SweepMultiArgs {
    int64_t count, blocks; // units, and unit blocks
    int s;
    const SweepUnit *units;
    const int32_t *colidx;
    const double *val, *wd, *b, *x;
    double *y;
    int64_t ldb, ldx, ldy;
};

// Every lane of the wave runs this together (the butterflies move data between lanes).  x and y are distinct blocks:
// other rows gather x while this one writes y.
template <int MODE, bool FAST> __device__ __forceinline__ void sweep_row_multi(const SweepMultiArgs &a, const SweepUnit u, int j0, unsigned mask)
{
    const int gs = sptrsv_group_shift((int64_t)u.end - u.beg);
    const int lane = 4 * u.q + (threadIdx.x & 3);
    const bool writer = u.row >= 0 && lane == 0;
    // what the row's last step needs travels with its first entries instead of waiting behind the fold
    double bi[TILE], xi[TILE];
#pragma unroll
    for (int c = 0; c < TILE; ++c) bi[c] = xi[c] = 0.0;
    double wi = 0.0;
    if (writer) {
        tile_ld<TILE, FAST>(a.b + (int64_t)u.row * a.ldb + j0, mask, bi);
        if constexpr (MODE == MODE_SWEEP) {
            tile_ld<TILE, FAST>(a.x + (int64_t)u.row * a.ldx + j0, mask, xi);
            wi = a.wd[u.row];
        }
    }
    double f[TILE];
    tile_row_sums<FAST>(u, gs, lane, a.colidx, a.val, a.x + j0, a.ldx, mask, f);
    if (writer) {
        double out[TILE];
#pragma unroll
        for (int c = 0; c < TILE; ++c) {
            const double d = bi[c] - f[c];
            if constexpr (MODE == MODE_RESIDUAL) {
                out[c] = d;
            } else {
                const double t = wi * d;
                out[c] = xi[c] + t;
            }
        }
        tile_st<TILE, FAST>(a.y + (int64_t)u.row * a.ldy + j0, mask, out);
    }
}

template <int MODE, bool WIDE> __global__ __launch_bounds__(AMG_THREADS) void amg_sweep_multi_kernel(const SweepMultiArgs a)
{
    const TileId id = tile_id(a.blocks, tiles(a.s));
    const int j0 = (int)id.tile * TILE, w = a.s - j0 < TILE ? a.s - j0 : TILE;
    const unsigned mask = (1u << w) - 1u;
    const SweepUnit u = multi_unit(id.block, a.count, a.units);
    if (WIDE && w == TILE) sweep_row_multi<MODE, true>(a, u, j0, mask);
    else sweep_row_multi<MODE, false>(a, u, j0, mask);
}

struct TransferMultiArgs {
    int64_t count, blocks;
    int s;
    const SweepUnit *units;
    const int32_t *colidx;
    const double *val;
    double scale;
    const double *in;
    double *out;
    int64_t ldin, ldout;
};

// transfer_row over a tile.  `out` is never gathered: the prolongation updates it in place.
template <int MODE, bool FAST> __device__ __forceinline__ void transfer_row_multi(const TransferMultiArgs &a, const SweepUnit u, int j0, unsigned mask)
{
    const int gs = sptrsv_group_shift((int64_t)u.end - u.beg);
    const int lane = 4 * u.q + (threadIdx.x & 3);
    const bool writer = u.row >= 0 && lane == 0;
    double xi[TILE];
#pragma unroll
    for (int c = 0; c < TILE; ++c) xi[c] = 0.0;
    if constexpr (MODE == AMG_PROLONG)
        if (writer) tile_ld<TILE, FAST>(a.out + (int64_t)u.row * a.ldout + j0, mask, xi); // travels with the first entries
    double f[TILE];
    tile_row_sums<FAST>(u, gs, lane, a.colidx, a.val, a.in + j0, a.ldin, mask, f);
    if (writer) {
        double out[TILE];
#pragma unroll
        for (int c = 0; c < TILE; ++c) {
            if constexpr (MODE == AMG_RESTRICT) {
                out[c] = f[c];
            } else {
                const double t = a.scale * f[c];
                out[c] = xi[c] + t;
            }
        }
        tile_st<TILE, FAST>(a.out + (int64_t)u.row * a.ldout + j0, mask, out);
    }
}

template <int MODE, bool WIDE> __global__ __launch_bounds__(AMG_THREADS) void amg_transfer_multi_kernel(const TransferMultiArgs a)
{
    const TileId id = tile_id(a.blocks, tiles(a.s));
    const int j0 = (int)id.tile * TILE, w = a.s - j0 < TILE ? a.s - j0 : TILE;
    const unsigned mask = (1u << w) - 1u;
    const SweepUnit u = multi_unit(id.block, a.count, a.units);
    if (WIDE && w == TILE) transfer_row_multi<MODE, true>(a, u, j0, mask);
    else transfer_row_multi<MODE, false>(a, u, j0, mask);
}

// the first sweep from a zero guess: Y[i, c] = wd[i] * B[i, c]; one thread an element, consecutive threads along a row
__global__ __launch_bounds__(AMG_THREADS) void amg_first_multi_kernel(int64_t n, int s, const double *__restrict__ wd, const double *__restrict__ b,
                                                                      int64_t ldb, double *__restrict__ y, int64_t ldy)
{
    const int64_t t = (int64_t)blockIdx.x * AMG_THREADS + threadIdx.x, i = t / s, c = t - i * s;
    if (i < n) y[i * ldy + c] = wd[i] * b[i * ldb + c];
}

// one thread an (aggregate, column), columns fastest so that a member's row is read contiguously; the members ascending,
// sequentially from +0
__global__ __launch_bounds__(AMG_THREADS) void amg_restrict_multi_kernel(int64_t n_agg, int s, const int32_t *__restrict__ aggptr,
                                                                         const int32_t *__restrict__ members, const double *__restrict__ res,
                                                                         int64_t ldr, double *__restrict__ bc, int64_t ldc)
{
    const int64_t t = (int64_t)blockIdx.x * AMG_THREADS + threadIdx.x, a = t / s, c = t - a * s;
    if (a >= n_agg) return;
    double sum = 0.0;
    for (int64_t k = aggptr[a]; k < aggptr[a + 1]; ++k) sum = sum + res[(int64_t)members[k] * ldr + c];
    bc[a * ldc + c] = sum;
}

// one thread a (row, column)
__global__ __launch_bounds__(AMG_THREADS) void amg_prolong_multi_kernel(int64_t n, int s, const int32_t *__restrict__ agg, double scale,
                                                                        const double *__restrict__ e, int64_t lde, double *__restrict__ x,
                                                                        int64_t ldx)
{
    const int64_t t = (int64_t)blockIdx.x * AMG_THREADS + threadIdx.x, i = t / s, c = t - i * s;
    if (i >= n) return;
    const double p = scale * e[(int64_t)agg[i] * lde + c];
    x[i * ldx + c] = x[i * ldx + c] + p;
}

// ---- launches ----------------------------------------------------------------------------------------------------------
// a grid that would not fit a launch is refused by the entries before anything is launched (amg.hip's multi_grids_ok)
inline unsigned amg_multi_grid_of(int64_t units, int s) { return (unsigned)tile_grid(unit_blocks(units, AMG_UNITS_PER_BLOCK), s); }

template <int MODE> inline void launch_sweep_multi_mode(hipStream_t st, const SweepMultiArgs &a)
{
    const bool wide = wide16(a.b, a.ldb) && wide16(a.x, a.ldx) && wide16(a.y, a.ldy);
    if (wide) amg_sweep_multi_kernel<MODE, true><<<amg_multi_grid_of(a.count, a.s), AMG_THREADS, 0, st>>>(a);
    else amg_sweep_multi_kernel<MODE, false><<<amg_multi_grid_of(a.count, a.s), AMG_THREADS, 0, st>>>(a);
}

template <int MODE> inline void launch_transfer_multi_mode(hipStream_t st, const TransferMultiArgs &a)
{
    const bool wide = wide16(a.in, a.ldin) && wide16(a.out, a.ldout);
    if (wide) amg_transfer_multi_kernel<MODE, true><<<amg_multi_grid_of(a.count, a.s), AMG_THREADS, 0, st>>>(a);
    else amg_transfer_multi_kernel<MODE, false><<<amg_multi_grid_of(a.count, a.s), AMG_THREADS, 0, st>>>(a);
}

} // namespace
