// unit_row.h -- the device text under every kernel that sums a stored row by four-lane units: the
// triangular solves (sptrsv.hip), the AMG sweeps and transfers (amg.hip), the Chebyshev step (cheby.hip), and their
// widenings by a tile of TILE columns (sptrsm_tile_kernels.h, amg_multi_kernels.h); the tile's load, store and workgroup
// numbering also serve krylov_multi.hip.  One definition each of the record, the tile's access, the numbering, the fold
// and the whole-row sum.
//
// Nothing in here can be contracted, whatever the including file's pragma says: the row sum calls __builtin_fma by name
// and everything else is an addition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rowwise.h"
#include "sptrsv.h"
#include "tile.h"

namespace sblas {

// Four lanes of a sweep launch (level_plan.h) over whole rows -- AMG's and the Chebyshev plan's; q: the unit's number in
// its row; a pad has row = -1.
struct SweepUnit {
    int32_t row, beg, end, q;
};
constexpr SweepUnit NO_SWEEP_UNIT{-1, 0, 0, 0};

// ---- a row's W columns, W even (the tile: W = TILE) ----------------------------------------------------------------------
// FAST: W / 2 16-byte accesses (the launch's alignment allows it, decided on the host by wide16(), and the tile is
// full).  Otherwise column by column under the mask: a column outside it is not touched and reads as 0.  Same values,
// same order, same bits.
template <int W, bool FAST> __device__ __forceinline__ void tile_ld(const double *p, unsigned mask, double (&x)[W])
{
    static_assert(W % 2 == 0, "the 16-byte path moves two columns an access");
    if constexpr (FAST) {
        const double2 *q = reinterpret_cast<const double2 *>(p);
#pragma unroll
        for (int c = 0; c < W / 2; ++c) {
            const double2 t = q[c];
            x[2 * c] = t.x, x[2 * c + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int c = 0; c < W; ++c) x[c] = (mask >> c & 1u) ? p[c] : 0.0;
    }
}

template <int W, bool FAST> __device__ __forceinline__ void tile_st(double *p, unsigned mask, const double (&x)[W])
{
    static_assert(W % 2 == 0, "the 16-byte path moves two columns an access");
    if constexpr (FAST) {
        double2 *q = reinterpret_cast<double2 *>(p);
#pragma unroll
        for (int c = 0; c < W / 2; ++c) q[c] = make_double2(x[2 * c], x[2 * c + 1]);
    } else {
#pragma unroll
        for (int c = 0; c < W; ++c)
            if (mask >> c & 1u) p[c] = x[c];
    }
}

// Which row block (a cell, a unit block) and which column tile a workgroup takes.  The grid is one-dimensional, blocks x
// tiles workgroups, numbered so that the tiles of one row block are TILE_GROUP ids apart and next to each other in time:
// row blocks go in groups of TILE_GROUP, and inside a group the id runs over the row blocks first, then over the tiles.
// At s > 8 two tiles of a row block read halves of the same memory lines (a row is s * 8 bytes, a tile 64 of them) and
// the same entries of A; workgroup ids that differ by the number of L2 partitions are dispatched to the same partition,
// so the second tile finds the lines the first one fetched.  The numbering cannot reach a bit: a (row block, tile) pair
// computes the same sums wherever it runs.
struct TileId {
    int64_t block, tile;
};
__device__ __forceinline__ TileId tile_id(int64_t blocks, int64_t tiles)
{
    const int64_t per = TILE_GROUP * tiles, id = blockIdx.x, g = id / per, rem = id - g * per;
    const int64_t left = blocks - TILE_GROUP * g, gb = left < TILE_GROUP ? left : TILE_GROUP; // the last group is short
    return TileId{TILE_GROUP * g + rem % gb, rem / gb};
}

// The sum over a row's 1 << gs lanes (gs = sptrsv_group_shift(p): 2, 4 or 6) of each lane's s, by the butterfly of
// rowwise.h.  Every lane of the wave calls this together, whatever its own row's gs; a row's lanes all return its sum.
__device__ __forceinline__ double group_fold(double s, int gs)
{
    const double f4 = fold_sum<4>(s);
    double f16 = f4 + lane_partner<4>(f4);
    f16 += lane_partner<8>(f16);
    double f64 = f16 + lane_partner<16>(f16);
    f64 += lane_partner<32>(f64);
    return gs == 2 ? f4 : gs == 4 ? f16 : f64;
}

// The sum of one whole stored row against a vector, AMG's and the Chebyshev step's: the sum over the entries e
// (beg .. end - 1) of val[e] * x[colidx[e]].  Lane `lane` of the row's 1 << gs lanes takes the entries lane, lane + G, ...
// in stored order with one fused multiply-add each from +0, and the lanes fold by group_fold.  Every lane of the wave
// calls this together; a pad's lanes (live = false) load nothing.  The solves (sptrsv.hip: a triangle predicate, x read
// and written in one launch) and the tile kernels (amg_multi_kernels.h, sptrsm_tile_kernels.h: eight columns abreast)
// keep this loop in their own text over group_fold.
__device__ __forceinline__ double unit_row_sum(bool live, int32_t beg, int32_t end, int lane, int gs, const int32_t *__restrict__ colidx,
                                               const double *__restrict__ val, const double *__restrict__ x)
{
    const int G = 1 << gs;
    double s = 0.0;
    if (live)
        for (int64_t e = (int64_t)beg + lane; e < end; e += G) s = __builtin_fma(val[e], x[colidx[e]], s);
    return group_fold(s, gs);
}

} // namespace sblas
