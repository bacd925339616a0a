// fsai.h -- what fsai.hip's kernel and fsai_rule.cpp's host rule agree on: the sizes, the unit record of
// a launch, the place of an entry in the packed triangle and the test a pivot has to pass.  No HIP in here: FSAI_HD is
// empty unless the including file sets it, so fsai_rule.cpp is testable on a CPU box.
#pragma once
#include <float.h>
#include <stdint.h>
#include "sptrsv.h"

#ifndef FSAI_HD
#define FSAI_HD
#endif

namespace sblas {

constexpr int FSAI_ROW_MAX = 64;  // the longest row of G: the order of the largest dense system, one wave's lanes
constexpr int FSAI_THREADS = 256; // a workgroup of the setup kernel: four waves, as the sweeps'

// A row of G with m entries is worked by the solves' G(m) lanes (sptrsv_group_shift: 4 up to 4 entries, 16 up to 32, a
// whole wave beyond) and owns the LDS of those lanes: FSAI_TRI_PER_LANE doubles a lane for the packed lower triangle of M,
// FSAI_VEC_PER_LANE doubles a lane for g and as many int32 for J.  The three tiers' needs, each within its lanes' share:
constexpr int FSAI_TRI_PER_LANE = 33;
constexpr int FSAI_VEC_PER_LANE = 2;
constexpr int fsai_triangle(int m) { return m * (m + 1) / 2; }
static_assert(fsai_triangle((int)SPTRSV_G4_MAX) <= 4 * FSAI_TRI_PER_LANE && SPTRSV_G4_MAX <= 4 * FSAI_VEC_PER_LANE, "the 4-lane tier");
static_assert(fsai_triangle((int)SPTRSV_G16_MAX) <= 16 * FSAI_TRI_PER_LANE && SPTRSV_G16_MAX <= 16 * FSAI_VEC_PER_LANE, "the 16-lane tier");
static_assert(fsai_triangle(FSAI_ROW_MAX) <= 64 * FSAI_TRI_PER_LANE && FSAI_ROW_MAX <= 64 * FSAI_VEC_PER_LANE, "the 64-lane tier");
constexpr int FSAI_LDS_BYTES = FSAI_THREADS * (FSAI_TRI_PER_LANE * 8 + FSAI_VEC_PER_LANE * 8 + FSAI_VEC_PER_LANE * 4);

// Four lanes of the launch (level_plan.h packs them as one wide level on G's rowptr): row i of G is val_G[beg .. end - 1];
// q: the unit's number in its row; a pad has row = -1.
struct FsaiUnit {
    int32_t row, beg, end, q;
};
constexpr FsaiUnit NO_FSAI_UNIT{-1, 0, 0, 0};

// M[p][q], q <= p, in the packed lower triangle: row after row, so that a row is contiguous
FSAI_HD inline int fsai_at(int p, int q) { return p * (p + 1) / 2 + q; }

// a pivot (and a diagonal entry of the fallback) goes on only when it is finite and > 0 (a NaN fails the comparison)
FSAI_HD inline bool fsai_positive(double v) { return v > 0.0 && v <= DBL_MAX; }

// max_row as create and the pattern function take it: 0 refuses a row above FSAI_ROW_MAX, 1 .. FSAI_ROW_MAX thins
inline bool fsai_max_row_ok(int max_row) { return max_row >= 0 && max_row <= FSAI_ROW_MAX; }

} // namespace sblas
