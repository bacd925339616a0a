// amg_multi.h -- the sizes amg.hip's multi-column kernels (amg_multi_kernels.h) and amg_rule.cpp's host rule agree on
// (DESIGN.md 3.30).  No HIP in here.
#pragma once
#include <stdint.h>
#include "../../include/sblas_hip.h"
#include "amg.h"
#include "krylov_multi.h"

namespace sblas {

// A workgroup of a multi-column row kernel takes AMG_THREADS / 4 units and a tile of AMG_MULTI_TILE consecutive columns:
// a lane holds eight doubles of the row its entry names (64 bytes, four 16-byte loads when the alignment allows).
constexpr int AMG_MULTI_TILE = SBLAS_AMG_MULTI_TILE;
static_assert(AMG_MULTI_TILE == 8, "the column mask of a tile is eight bits and the wide path four 16-byte accesses");
static_assert(AMG_MULTI_TILE == KRYLOV_MULTI_TILE && SBLAS_AMG_MULTI_MAX_RHS == SBLAS_KRYLOV_MULTI_MAX_RHS, "the solvers' blocks are the cycle's");
constexpr int AMG_UNITS_PER_BLOCK = AMG_THREADS / 4;
// Unit blocks go in groups of AMG_MULTI_GROUP; inside a group the workgroup id runs over the unit blocks first, then
// over the tiles (krylov_multi.hip's tile_id): the tiles of one unit block are AMG_MULTI_GROUP ids apart, so they are
// dispatched to the same L2 partition next to each other in time and the later ones find A's entries there.
constexpr int AMG_MULTI_GROUP = 8;

inline bool amg_multi_width_ok(int64_t s) { return s >= 1 && s <= SBLAS_AMG_MULTI_MAX_RHS; }
constexpr int amg_multi_tiles(int s) { return (s + AMG_MULTI_TILE - 1) / AMG_MULTI_TILE; }
constexpr int64_t amg_multi_unit_blocks(int64_t units) { return (units + AMG_UNITS_PER_BLOCK - 1) / AMG_UNITS_PER_BLOCK; }

} // namespace sblas
