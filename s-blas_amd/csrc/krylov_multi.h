// krylov_multi.h -- the sizes krylov_multi.hip's kernels and krylov_multi_rule.cpp's host rule agree on.  No HIP in here.
#pragma once
#include <stdint.h>
#include "../../include/sblas_hip.h"
#include "krylov.h"
#include "tile.h"

namespace sblas {

// One workgroup takes a cell of KRYLOV_CELL rows and a tile of TILE consecutive columns (tile.h).
static_assert(SBLAS_KRYLOV_MULTI_MAX_RHS % TILE == 0, "the widest batch is whole tiles");

// n is at most INT_MAX and s at most SBLAS_KRYLOV_MULTI_MAX_RHS (both refused before any launch), so no grid of cells x
// tiles reaches tile_grid()'s refusal: the launches cast its result
static_assert(tile_grid(((int64_t)INT_MAX + KRYLOV_CELL - 1) / KRYLOV_CELL, SBLAS_KRYLOV_MULTI_MAX_RHS) > 0, "the widest grid fits a launch");

inline bool krylov_multi_width_ok(int64_t s) { return s >= 1 && s <= SBLAS_KRYLOV_MULTI_MAX_RHS; }

} // namespace sblas
