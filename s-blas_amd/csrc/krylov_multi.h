// krylov_multi.h -- the sizes krylov_multi.hip's kernels and krylov_multi_rule.cpp's host rule agree on.  No HIP in here.
#pragma once
#include <stddef.h>
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

// the bytes an n x s block at leading dimension ld spans
inline size_t span_bytes(int64_t n, int s, int64_t ld) { return n > 0 ? ((size_t)(n - 1) * (size_t)ld + (size_t)s) * 8 : 0; }
// what start refuses as "X overlaps B": the spans of two n x s blocks at x0 and b0 share a byte.  Spans, not entries: the
// two column halves of one (n, 2s) tensor interleave without sharing an entry and are refused all the same
inline bool blocks_overlap(uintptr_t x0, int64_t ldx, uintptr_t b0, int64_t ldb, int64_t n, int s)
{
    return b0 < x0 + span_bytes(n, s, ldx) && x0 < b0 + span_bytes(n, s, ldb);
}

} // namespace sblas
