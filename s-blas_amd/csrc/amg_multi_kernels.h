// amg_multi_kernels.h -- amg.hip's kernels widened by a tile of AMG_MULTI_TILE columns: the block cycle
// Z = M^-1 R on n x s row-major blocks.  Included by amg.hip alone, after its Unit, its modes and its single-column
// kernels, whose text this file restates column by column:
//   sweep / residual   sweep_row over a tile: a lane fetches val[e] and colidx[e] ONCE per entry and then the eight
//                      doubles X[col * ldx + j0 .. j0 + 7]; eight accumulators, eight butterflies; the writer lane reads
//                      b, x, wd for its row and tile and stores eight doubles;
//   transfer           transfer_row widened the same way (a smoothed plan's R_l and P_l);
//   first, restrict, prolong   one thread per (row or aggregate, column), columns fastest.
// Column c of a tile goes through exactly the operations of the single kernel in the same order -- one fused
// multiply-add per entry from +0 in the lane order of G(p), the butterfly of rowwise.h, then the row's last step rounded
// operation by operation (contraction is off at amg.hip's file scope, ahead of this include) -- so column j of a block
// has the single kernel's bits on that column.  No column's value enters another column's arithmetic.
//
// Width of the accesses.  FAST: a full tile whose launch has every base and leading dimension a multiple of 16 bytes
// (decided on the host) moves a row's eight doubles as four 16-byte accesses.  Anything else -- the ragged last tile, an
// odd leading dimension, a base offset by one element -- goes double by double under the column mask; a column outside
// the mask is neither read nor written.  Same values, same order, same bits.
//
// No LDS, no atomics, nothing waits across workgroups.
#pragma once
#include <type_traits>
#include "amg_multi.h"

namespace {

constexpr int MT = AMG_MULTI_TILE;

template <bool FAST> __device__ __forceinline__ void amg_ld8(const double *p, unsigned mask, double (&x)[MT])
{
    if constexpr (FAST) {
        const double2 *q = reinterpret_cast<const double2 *>(p);
#pragma unroll
        for (int c = 0; c < MT / 2; ++c) {
            const double2 t = q[c];
            x[2 * c] = t.x, x[2 * c + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int c = 0; c < MT; ++c) x[c] = (mask >> c & 1u) ? p[c] : 0.0;
    }
}

template <bool FAST> __device__ __forceinline__ void amg_st8(double *p, unsigned mask, const double (&x)[MT])
{
    if constexpr (FAST) {
        double2 *q = reinterpret_cast<double2 *>(p);
#pragma unroll
        for (int c = 0; c < MT / 2; ++c) q[c] = make_double2(x[2 * c], x[2 * c + 1]);
    } else {
#pragma unroll
        for (int c = 0; c < MT; ++c)
            if (mask >> c & 1u) p[c] = x[c];
    }
}

// Which unit block and which column tile a workgroup takes: amg_multi.h's numbering.  It cannot reach a bit: a (unit,
// tile) pair computes the same sums wherever it runs.
struct AmgTileId {
    int64_t block;
    int tile;
};
__device__ __forceinline__ AmgTileId amg_tile_id(int64_t blocks, int s)
{
    const int64_t per = (int64_t)AMG_MULTI_GROUP * amg_multi_tiles(s), id = blockIdx.x, g = id / per, rem = id - g * per;
    const int64_t left = blocks - AMG_MULTI_GROUP * g, gb = left < AMG_MULTI_GROUP ? left : AMG_MULTI_GROUP; // the last group is short
    return AmgTileId{AMG_MULTI_GROUP * g + rem % gb, (int)(rem / gb)};
}

// wide_unit() with the unit block given instead of read off blockIdx.x
__device__ __forceinline__ Unit multi_unit(int64_t block, int64_t count, const Unit *__restrict__ units)
{
    const int64_t u = (block * AMG_THREADS + threadIdx.x) >> 2;
    return u < count ? load_unit(units, u) : NO_UNIT;
}

// the row sums of a tile: sweep_row's loop and fold, eight columns abreast; the writer lane's f[c] is column c's sum
template <bool FAST>
__device__ __forceinline__ void tile_row_sums(const Unit u, int gs, int lane, const int32_t *__restrict__ colidx, const double *__restrict__ val,
                                              const double *__restrict__ x, int64_t ldx, unsigned mask, double (&f)[MT])
{
    const int G = 1 << gs;
    double s[MT];
#pragma unroll
    for (int c = 0; c < MT; ++c) s[c] = 0.0;
    if (u.row >= 0)
        for (int64_t e = (int64_t)u.beg + lane; e < u.end; e += G) {
            const double a = val[e];
            double xv[MT];
            amg_ld8<FAST>(x + (int64_t)colidx[e] * ldx, mask, xv);
#pragma unroll
            for (int c = 0; c < MT; ++c) s[c] = __builtin_fma(a, xv[c], s[c]);
        }
#pragma unroll
    for (int c = 0; c < MT; ++c) {
        const double f4 = fold_sum<4>(s[c]);
        double f16 = f4 + lane_partner<4>(f4);
        f16 += lane_partner<8>(f16);
        double f64 = f16 + lane_partner<16>(f16);
        f64 += lane_partner<32>(f64);
        f[c] = gs == 2 ? f4 : gs == 4 ? f16 : f64;
    }
}

struct SweepMultiArgs {
    int64_t count, blocks; // units, and unit blocks
    int s;
    const Unit *units;
    const int32_t *colidx;
    const double *val, *wd, *b, *x;
    double *y;
    int64_t ldb, ldx, ldy;
};

// Every lane of the wave runs this together (the butterflies move data between lanes).  x and y are distinct blocks:
// other rows gather x while this one writes y.
template <int MODE, bool FAST> __device__ __forceinline__ void sweep_row_multi(const SweepMultiArgs &a, const Unit u, int j0, unsigned mask)
{
    const int gs = sptrsv_group_shift((int64_t)u.end - u.beg);
    const int lane = 4 * u.q + (threadIdx.x & 3);
    const bool writer = u.row >= 0 && lane == 0;
    // what the row's last step needs travels with its first entries instead of waiting behind the fold
    double bi[MT], xi[MT];
#pragma unroll
    for (int c = 0; c < MT; ++c) bi[c] = xi[c] = 0.0;
    double wi = 0.0;
    if (writer) {
        amg_ld8<FAST>(a.b + (int64_t)u.row * a.ldb + j0, mask, bi);
        if constexpr (MODE == MODE_SWEEP) {
            amg_ld8<FAST>(a.x + (int64_t)u.row * a.ldx + j0, mask, xi);
            wi = a.wd[u.row];
        }
    }
    double f[MT];
    tile_row_sums<FAST>(u, gs, lane, a.colidx, a.val, a.x + j0, a.ldx, mask, f);
    if (writer) {
        double out[MT];
#pragma unroll
        for (int c = 0; c < MT; ++c) {
            const double d = bi[c] - f[c];
            if constexpr (MODE == MODE_RESIDUAL) {
                out[c] = d;
            } else {
                const double t = wi * d;
                out[c] = xi[c] + t;
            }
        }
        amg_st8<FAST>(a.y + (int64_t)u.row * a.ldy + j0, mask, out);
    }
}

template <int MODE, bool WIDE> __global__ __launch_bounds__(AMG_THREADS) void amg_sweep_multi_kernel(const SweepMultiArgs a)
{
    const AmgTileId id = amg_tile_id(a.blocks, a.s);
    const int j0 = id.tile * MT, w = a.s - j0 < MT ? a.s - j0 : MT;
    const unsigned mask = (1u << w) - 1u;
    const Unit u = multi_unit(id.block, a.count, a.units);
    if (WIDE && w == MT) sweep_row_multi<MODE, true>(a, u, j0, mask);
    else sweep_row_multi<MODE, false>(a, u, j0, mask);
}

struct TransferMultiArgs {
    int64_t count, blocks;
    int s;
    const Unit *units;
    const int32_t *colidx;
    const double *val;
    double scale;
    const double *in;
    double *out;
    int64_t ldin, ldout;
};

// transfer_row over a tile.  `out` is never gathered: the prolongation updates it in place.
template <int MODE, bool FAST> __device__ __forceinline__ void transfer_row_multi(const TransferMultiArgs &a, const Unit u, int j0, unsigned mask)
{
    const int gs = sptrsv_group_shift((int64_t)u.end - u.beg);
    const int lane = 4 * u.q + (threadIdx.x & 3);
    const bool writer = u.row >= 0 && lane == 0;
    double xi[MT];
#pragma unroll
    for (int c = 0; c < MT; ++c) xi[c] = 0.0;
    if constexpr (MODE == AMG_PROLONG)
        if (writer) amg_ld8<FAST>(a.out + (int64_t)u.row * a.ldout + j0, mask, xi); // travels with the first entries
    double f[MT];
    tile_row_sums<FAST>(u, gs, lane, a.colidx, a.val, a.in + j0, a.ldin, mask, f);
    if (writer) {
        double out[MT];
#pragma unroll
        for (int c = 0; c < MT; ++c) {
            if constexpr (MODE == AMG_RESTRICT) {
                out[c] = f[c];
            } else {
                const double t = a.scale * f[c];
                out[c] = xi[c] + t;
            }
        }
        amg_st8<FAST>(a.out + (int64_t)u.row * a.ldout + j0, mask, out);
    }
}

template <int MODE, bool WIDE> __global__ __launch_bounds__(AMG_THREADS) void amg_transfer_multi_kernel(const TransferMultiArgs a)
{
    const AmgTileId id = amg_tile_id(a.blocks, a.s);
    const int j0 = id.tile * MT, w = a.s - j0 < MT ? a.s - j0 : MT;
    const unsigned mask = (1u << w) - 1u;
    const Unit u = multi_unit(id.block, a.count, a.units);
    if (WIDE && w == MT) transfer_row_multi<MODE, true>(a, u, j0, mask);
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
inline bool amg_wide16(const void *p, int64_t ld) { return ((reinterpret_cast<uintptr_t>(p) | (uintptr_t)(ld * 8)) & 15u) == 0; }
inline unsigned amg_multi_grid_of(int64_t units, int s) { return (unsigned)(amg_multi_unit_blocks(units) * amg_multi_tiles(s)); }

template <int MODE> inline void launch_sweep_multi_mode(hipStream_t st, const SweepMultiArgs &a)
{
    const bool wide = amg_wide16(a.b, a.ldb) && amg_wide16(a.x, a.ldx) && amg_wide16(a.y, a.ldy);
    if (wide) amg_sweep_multi_kernel<MODE, true><<<amg_multi_grid_of(a.count, a.s), AMG_THREADS, 0, st>>>(a);
    else amg_sweep_multi_kernel<MODE, false><<<amg_multi_grid_of(a.count, a.s), AMG_THREADS, 0, st>>>(a);
}

template <int MODE> inline void launch_transfer_multi_mode(hipStream_t st, const TransferMultiArgs &a)
{
    const bool wide = amg_wide16(a.in, a.ldin) && amg_wide16(a.out, a.ldout);
    if (wide) amg_transfer_multi_kernel<MODE, true><<<amg_multi_grid_of(a.count, a.s), AMG_THREADS, 0, st>>>(a);
    else amg_transfer_multi_kernel<MODE, false><<<amg_multi_grid_of(a.count, a.s), AMG_THREADS, 0, st>>>(a);
}

} // namespace
