// krylov_multi.h -- the sizes krylov_multi.hip's kernels and krylov_multi_rule.cpp's host rule agree on.  No HIP in here.
#pragma once
#include <stdint.h>
#include "../../include/sblas_hip.h"
#include "krylov.h"

namespace sblas {

// One workgroup takes a cell of KRYLOV_CELL rows and a tile of KRYLOV_MULTI_TILE consecutive columns: a lane holds its
// row's eight doubles of each operand (64 bytes, four 16-byte loads when the alignment allows).
constexpr int KRYLOV_MULTI_TILE = SBLAS_KRYLOV_MULTI_TILE;
static_assert(KRYLOV_MULTI_TILE == 8, "the status mask of a tile is eight bits and the wide path four 16-byte accesses");
static_assert(SBLAS_KRYLOV_MULTI_MAX_RHS % KRYLOV_MULTI_TILE == 0, "the widest batch is whole tiles");

inline bool krylov_multi_width_ok(int64_t s) { return s >= 1 && s <= SBLAS_KRYLOV_MULTI_MAX_RHS; }
inline int krylov_multi_tiles(int s) { return (s + KRYLOV_MULTI_TILE - 1) / KRYLOV_MULTI_TILE; }

} // namespace sblas
