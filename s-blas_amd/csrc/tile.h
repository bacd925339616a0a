// tile.h -- the column tile every widened kernel and its host rule agree on: the multi-right-hand-side
// Krylov updates (krylov_multi.hip), the block AMG cycle (amg_multi_kernels.h) and the tiled SpSM (sptrsm_tile_kernels.h)
// all work on n x s row-major blocks, TILE consecutive columns a workgroup.  No HIP in here: the rules that call it are
// testable on a CPU box.
#pragma once
#include <limits.h>
#include <stdint.h>
#include "../../include/sblas_hip.h"

namespace sblas {

// A lane holds its row's eight doubles of each operand: 64 bytes, four 16-byte accesses when the alignment allows, and
// the column mask of a tile is eight bits.
constexpr int TILE = 8;
static_assert(SBLAS_KRYLOV_MULTI_TILE == TILE && SBLAS_AMG_MULTI_TILE == TILE && SBLAS_SPTRSM_TILE == TILE, "one tile width under every family");
// Row blocks (cells, unit blocks) go in groups of TILE_GROUP; inside a group the workgroup id runs over the row blocks
// first, then over the tiles (unit_row.h's tile_id): the tiles of one row block are TILE_GROUP ids apart.
constexpr int TILE_GROUP = 8;
constexpr int64_t TILE_MAX_GRID = INT_MAX; // workgroups of one launch

constexpr int64_t tiles(int64_t s) { return s / TILE + (s % TILE != 0); } // no sum that could wrap
constexpr int tiles(int s) { return (s + TILE - 1) / TILE; }                 // a width the public limits bound: 32-bit arithmetic
// row blocks of `per_block` units each that cover `units` units
constexpr int64_t unit_blocks(int64_t units, int64_t per_block) { return units / per_block + (units % per_block != 0); }
// workgroups of a launch of `blocks` row blocks for s >= 1 columns, -1 where they pass TILE_MAX_GRID
constexpr int64_t tile_grid(int64_t blocks, int64_t s)
{
    if (tiles(s) > TILE_MAX_GRID) return -1;
    return blocks == 0 || tiles(s) <= TILE_MAX_GRID / blocks ? blocks * tiles(s) : -1;
}
// a block at base p with leading dimension ld (doubles) takes the 16-byte accesses: every row's tile starts on one
inline bool wide16(const void *p, int64_t ld) { return ((reinterpret_cast<uintptr_t>(p) | (uintptr_t)(ld * 8)) & 15u) == 0; }

} // namespace sblas
