// sptrsv.h -- the sizes sptrsv.hip's kernels and sptrsv_plan.cpp's host rule agree on.  No HIP in here: sptrsv_plan.cpp is
// testable on a CPU box.
#pragma once
#include <stdint.h>

namespace sblas {

// The chain kernel is one workgroup of this many threads: 256 rows of the narrowest group in one pass.
constexpr int SPTRSV_CHAIN_THREADS = 1024;
// A level of at most this many rows is "narrow" (default of chain_rows): it joins a chain launch under
// SBLAS_SPTRSV_AUTO.  Chosen from the sweep in profiles/r12_sptrsv.json: the largest value at which
// `auto` is not slower than `per_level` on any of the five bench matrices.  The rule counts rows, while the chain
// workgroup's capacity is in lanes (256 rows of four lanes a pass, or 16 whole-wave rows): on the power-law triangle the
// narrow levels hold the longest rows, and from 64 on they take several passes each.
constexpr int64_t SPTRSV_CHAIN_ROWS = 32;
// G(p): lanes that share a row of p stored entries (the whole stored row counts, whichever triangle an entry is in).
constexpr int64_t SPTRSV_G4_MAX = 4;   // p <= 4: 4 lanes, one entry each
constexpr int64_t SPTRSV_G16_MAX = 32; // p <= 32: 16 lanes, up to two entries each; beyond: a whole wave
constexpr int sptrsv_group_shift(int64_t p) { return p <= SPTRSV_G4_MAX ? 2 : p <= SPTRSV_G16_MAX ? 4 : 6; }

} // namespace sblas
