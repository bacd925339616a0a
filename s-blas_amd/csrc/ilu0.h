// ilu0.h -- the sizes ilu0.hip's kernels and ilu0_plan.cpp's host rule agree on, and the kernels' unit record.
// No HIP in here: ilu0_plan.cpp is testable on a CPU box.
#pragma once
#include <stdint.h>
#include "sptrsv.h"

namespace sblas {

// The chain kernel is one workgroup of this many threads, as the solves' is.  Its LDS (ILU0_LDS_PER_LANE entries of
// 12 bytes a lane: 48 KB) fits the 160 KB of a CU three times over, so the size was not cut.
constexpr int ILU0_CHAIN_THREADS = SPTRSV_CHAIN_THREADS;
constexpr int ILU0_WIDE_THREADS = 256;
// A level of at most this many rows joins a chain launch under SBLAS_SPTRSV_AUTO (default of chain_rows).  It starts as
// the solves' default and is UNMEASURED for the factorisation: a factored row costs far more than a solved one, so the
// best value is likely lower.  Change it only from a sweep of tools/ilu0_bench.py.
constexpr int64_t ILU0_CHAIN_ROWS = SPTRSV_CHAIN_ROWS;
// G(p), the lanes that share a row of p stored entries, is the solves': sptrsv_group_shift().  A lane brings
// ILU0_LDS_PER_LANE entries of LDS, so a row's slice holds 4 * G(p) entries: 16 for p <= 4, 64 for p <= 32, and 256 for a
// whole wave.  A row of more than ILU0_LDS_MAX stored entries is on the long tier and works in lu itself.
constexpr int ILU0_LDS_PER_LANE = 4;
constexpr int64_t ILU0_LDS_MAX = 64 * ILU0_LDS_PER_LANE;
static_assert(SPTRSV_G4_MAX <= 4 * ILU0_LDS_PER_LANE && SPTRSV_G16_MAX <= 16 * ILU0_LDS_PER_LANE, "a row fits its group's slice");

// ILU(0)'s unit record (level_plan.h): every unit of a row carries the row's record; a unit that pads has row = -1.
struct Ilu0Unit {
    int32_t row, beg, diag, end; // the row's extent in val and the position of its diagonal
};

} // namespace sblas
