// geam.h -- the sizes geam.hip's kernels and its launches agree on.  No HIP in here.
#pragma once
#include <stdint.h>

namespace sblas {

constexpr int GEAM_THREADS = 256;          // a workgroup of the entry-parallel passes takes this many consecutive entries
constexpr int64_t GEAM_SORTED_LAUNCHES = 1; // one numeric on the sorted path: one launch over C's entries
constexpr int64_t GEAM_GENERAL_LAUNCHES = 2; // on the general path: the scaled values, then the COO plan's assemble; the ordered scatter's two

} // namespace sblas
