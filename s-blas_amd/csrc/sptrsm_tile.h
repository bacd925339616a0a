// sptrsm_tile.h -- the sizes sptrsv.hip's tiled SpSM kernels (sptrsm_tile_kernels.h) and the host rule in sptrsv_plan.cpp
// agree on.  No HIP in here.
#pragma once
#include <stdint.h>
#include "../../include/sblas_hip.h"
#include "sptrsv.h"
#include "tile.h"

namespace sblas {

// A workgroup of the tiled solve's wide launch takes a unit block of SPTRSM_WIDE_THREADS / 4 units, four lanes each as in
// the single solve, and a tile of TILE consecutive columns (tile.h); a chain launch is the wide launch of one unit block.
constexpr int SPTRSM_WIDE_THREADS = 256; // sptrsv.hip's WIDE_THREADS
constexpr int SPTRSM_UNITS_PER_BLOCK = SPTRSM_WIDE_THREADS / 4;
constexpr int64_t SPTRSM_MAX_GRID = TILE_MAX_GRID; // workgroups of one launch: what tile_grid() refuses to pass

} // namespace sblas
