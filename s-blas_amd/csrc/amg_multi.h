// amg_multi.h -- the sizes amg.hip's multi-column kernels (amg_multi_kernels.h) and amg_rule.cpp's host rule agree on
// (DESIGN.md 3.30).  No HIP in here.
#pragma once
#include <stdint.h>
#include "../../include/sblas_hip.h"
#include "amg.h"
#include "tile.h"

namespace sblas {

// A workgroup of a multi-column row kernel takes a unit block of AMG_THREADS / 4 units and a tile of TILE consecutive
// columns (tile.h).
static_assert(SBLAS_AMG_MULTI_MAX_RHS == SBLAS_KRYLOV_MULTI_MAX_RHS, "the solvers' blocks are the cycle's");
constexpr int AMG_UNITS_PER_BLOCK = AMG_THREADS / 4;

inline bool amg_multi_width_ok(int64_t s) { return s >= 1 && s <= SBLAS_AMG_MULTI_MAX_RHS; }

} // namespace sblas
