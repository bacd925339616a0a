// color.h -- the sizes color.hip's kernels and color_rule.cpp's host rule agree on, the priority hash both evaluate, and
// the host rule's internal interface.  No HIP in here: color_rule.cpp is testable on a CPU box.
#pragma once
#include <stdint.h>
#include <vector>
#include "sptrsv.h"

#if defined(__HIPCC__)
#define SBLAS_COLOR_HD __host__ __device__
#else
#define SBLAS_COLOR_HD
#endif

namespace sblas {

// A vertex of p = len(row v of A) + len(row v of A^T) stored entries belongs to the solves' G(p) lanes
// (sptrsv_group_shift): 4 lanes up to COLOR_G4_MAX, 16 up to COLOR_G16_MAX, a whole wave beyond.
constexpr int64_t COLOR_G4_MAX = SPTRSV_G4_MAX;
constexpr int64_t COLOR_G16_MAX = SPTRSV_G16_MAX;
// One pass of the round kernel sees the colours [w * COLOR_WINDOW, (w + 1) * COLOR_WINDOW): one bit a colour in a 64-bit
// mask per lane.
constexpr int COLOR_WINDOW = 64;
constexpr int COLOR_THREADS = 256; // a round workgroup: four waves

// fmix32 (the 32-bit finaliser of MurmurHash3): a bijection on 32-bit words
SBLAS_COLOR_HD inline uint32_t color_fmix32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}
// h(v) = fmix32(v + salt) with salt = 0x9E3779B9 * (seed + 1), all in wrapping uint32: no two vertices tie
inline uint32_t color_salt(uint32_t seed) { return 0x9E3779B9u * (seed + 1u); }
SBLAS_COLOR_HD inline uint32_t color_priority(uint32_t v, uint32_t salt) { return color_fmix32(v + salt); }

// The structure check of sblas_csr_color on host arrays, and with it the pattern of A^T (tptr: n + 1, tidx: nnz; column c
// of A lists its rows ascending).  SBLAS_OK or SBLAS_E_INVALID with the first bad row.
int color_check_transpose(int64_t n, const int32_t *rowptr, const int32_t *colidx, std::vector<int32_t> &tptr,
                          std::vector<int32_t> &tidx, int64_t *bad_row);

} // namespace sblas
