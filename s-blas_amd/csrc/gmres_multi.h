// gmres_multi.h -- the sizes gmres_multi.hip's kernels and gmres_multi_rule.cpp's host rule agree on.  No HIP in here.
// The cell and the tile are krylov_multi.h's, the two device blocks of a column are gmres.h's.
#pragma once
#include <stdint.h>
#include "../../include/sblas_hip.h"
#include "gmres.h"
#include "krylov_multi.h"

namespace sblas {

static_assert(SBLAS_GMRES_MULTI_MAX_RHS == SBLAS_KRYLOV_MULTI_MAX_RHS && SBLAS_GMRES_MULTI_TILE == TILE, "one batch width and one tile under both plans");
static_assert(SBLAS_GMRES_MULTI_MAX_RESTART == GMRES_MAX_RESTART, "the single solver's restart limit");

constexpr int GMRES_MULTI_FIXED_BLOCKS = 3; // W, U, Z beside the m + 1 blocks of V (a kind that cannot run in place adds one)
// column c's scalar block at scalars + GMRES_BLOCK_SLOTS * c, its small-matrix block at matrices + GMRES_MULTI_MATRIX_STRIDE * c
constexpr int64_t GMRES_MULTI_MATRIX_STRIDE = GMRES_MATRIX_DOUBLES;

inline bool gmres_multi_width_ok(int64_t s) { return krylov_multi_width_ok(s); }
inline bool gmres_multi_restart_ok(int64_t m) { return m >= 1 && m <= GMRES_MAX_RESTART; }

} // namespace sblas
