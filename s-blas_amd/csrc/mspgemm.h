// mspgemm.h -- the sizes mspgemm.hip's kernels, its launches and mspgemm_rule.cpp's limits agree on.  No HIP in here.
#pragma once
#include <stdint.h>

namespace sblas {

constexpr int MSPGEMM_THREADS = 256;      // a workgroup takes this many consecutive mask entries, a lane each
constexpr int MSPGEMM_WAVES = MSPGEMM_THREADS / 64;
constexpr int MSPGEMM_LDS_ROW = 256;      // the longest X row (entries) a wave stages: 12 bytes an entry, 12 KiB a workgroup
constexpr int64_t MSPGEMM_LAUNCHES = 1;   // one numeric is one launch over the mask's entries, on either path

} // namespace sblas
