// sptrsm_tile.h -- the sizes sptrsv.hip's tiled SpSM kernels (sptrsm_tile_kernels.h) and the host rule in sptrsv_plan.cpp
// agree on.  No HIP in here.
#pragma once
#include <limits.h>
#include <stdint.h>
#include "../../include/sblas_hip.h"
#include "krylov_multi.h"
#include "sptrsv.h"

namespace sblas {

// A workgroup of the tiled solve takes units of four lanes, as the single solve does, and a tile of SPTRSM_TILE consecutive
// columns: a lane holds eight doubles of the row its entry names (64 bytes, four 16-byte loads when the alignment allows).
constexpr int SPTRSM_TILE = SBLAS_SPTRSM_TILE;
static_assert(SPTRSM_TILE == 8, "the column mask of a tile is eight bits and the wide path four 16-byte accesses");
static_assert(SPTRSM_TILE == KRYLOV_MULTI_TILE, "the solvers' blocks are the solve's");
constexpr int SPTRSM_WIDE_THREADS = 256; // sptrsv.hip's WIDE_THREADS
constexpr int SPTRSM_UNITS_PER_BLOCK = SPTRSM_WIDE_THREADS / 4;
// Unit blocks of a wide level go in groups of SPTRSM_GROUP; inside a group the workgroup id runs over the unit blocks
// first, then over the tiles (amg_multi.h's numbering): the tiles of one unit block are SPTRSM_GROUP ids apart, next to
// each other in time, and the later ones find the row's entries in L2.
constexpr int SPTRSM_GROUP = 8;
constexpr int64_t SPTRSM_MAX_GRID = INT_MAX; // workgroups of one launch

constexpr int64_t sptrsm_tiles(int64_t s) { return s / SPTRSM_TILE + (s % SPTRSM_TILE != 0); } // no sum that could wrap
constexpr int64_t sptrsm_unit_blocks(int64_t units) { return units / SPTRSM_UNITS_PER_BLOCK + (units % SPTRSM_UNITS_PER_BLOCK != 0); }
// workgroups of a wide launch over `units` units for s >= 1 columns, -1 where they pass SPTRSM_MAX_GRID; a chain launch
// is the wide launch of one unit block
inline int64_t sptrsm_tile_grid(int64_t units, int64_t s)
{
    const int64_t blocks = sptrsm_unit_blocks(units), tiles = sptrsm_tiles(s);
    if (tiles > SPTRSM_MAX_GRID) return -1;
    return blocks == 0 || tiles <= SPTRSM_MAX_GRID / blocks ? blocks * tiles : -1;
}

} // namespace sblas
