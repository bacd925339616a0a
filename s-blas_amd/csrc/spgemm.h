// spgemm.h -- the sizes spgemm.hip's kernels and spgemm_plan.cpp's host rule agree on, and the rule's internal entry
// points.  No HIP in here: spgemm_plan.cpp is testable on a CPU box.
#pragma once
#include <stdint.h>

namespace sblas {

// The row path's LDS, per wave (a workgroup is one wave): a bitmap over the row's column span, the popcount prefix of
// its words and the accumulators -- 4 + 4 + 8 KiB = 16 KiB, ten waves a CU out of 160 KiB.
constexpr int64_t SPGEMM_S_MAX = 32768;                              // widest column span of a row-path row (bitmap bits)
constexpr int64_t SPGEMM_ACC_CAP = 1024;                             // C-row entries accumulated in LDS (64-lane form)
constexpr int SPGEMM_NARROW = 16;                                    // lanes of the narrow form: four rows to a wave
constexpr int64_t SPGEMM_NARROW_MEAN = 16;                           // narrow while products <= this * the A row's entries
constexpr int64_t SPGEMM_NARROW_S_MAX = SPGEMM_S_MAX / (64 / SPGEMM_NARROW); // each narrow group has a quarter of the LDS
constexpr int64_t SPGEMM_NARROW_ACC_CAP = SPGEMM_ACC_CAP / (64 / SPGEMM_NARROW);
constexpr int64_t SPGEMM_CHUNK_CAP = (int64_t)1 << 21;               // products of one general-path chunk (default)

} // namespace sblas
