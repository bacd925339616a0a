// sddmm_narrow.h -- what the narrow SDDMM's kernel (sddmm_narrow.hip) and its host rule (sddmm_narrow_rule.cpp) share: the
// sizes the kernel is built on, the part test and the dot product in the contract's order (include/sblas_hip_sddmm_narrow.h,
// (V)).  One definition each, plain C++ that compiles with and without HIP: the rule file is built alone under a host
// sanitizer (tools/sddmm_narrow_rule_check.cpp).
#pragma once
#include <stdint.h>
#include "../../include/sblas_hip.h"

#ifdef __HIPCC__
#define SBLAS_NARROW_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SBLAS_NARROW_HD inline
#endif

// every product below is rounded where it is written (for the rest of the two files that include this one)
#pragma clang fp contract(off)

namespace sblas {

constexpr int SDDMM_NARROW_MAX_K = 8;
constexpr int SDDMM_NARROW_THREADS = 256;
constexpr int SDDMM_NARROW_EPL = 4;                                              // consecutive entries one lane owns
constexpr int SDDMM_NARROW_CHUNK = SDDMM_NARROW_THREADS * SDDMM_NARROW_EPL;      // entries one workgroup takes

// elements of a row as the sum sees it: the k real ones, then +0 up to here (what sddmm_kernel's masked pieces hold)
constexpr int sddmm_narrow_padded(int k) { return k <= 2 ? 2 : k <= 4 ? 4 : 8; }

SBLAS_NARROW_HD bool sddmm_narrow_part_ok(int part) { return part >= SBLAS_PART_ALL && part <= SBLAS_PART_STRICT_UPPER; }
SBLAS_NARROW_HD bool sddmm_narrow_in_part(int part, int r, int c)
{
    return part == SBLAS_PART_ALL || (part == SBLAS_PART_LOWER && c <= r) || (part == SBLAS_PART_UPPER && c >= r) ||
           (part == SBLAS_PART_STRICT_LOWER && c < r) || (part == SBLAS_PART_STRICT_UPPER && c > r);
}

// <x, y> over kp = sddmm_narrow_padded(k) elements, the tail of both +0.  kp <= 4 is sddmm_kernel<1, kp / 2>: one lane,
// pieces in turn.  kp == 8 is sddmm_kernel<2, 2>: lane 0 takes the pieces 0 and 2 (elements 0, 1, 4, 5), lane 1 the pieces
// 1 and 3 (elements 2, 3, 6, 7), then one add.  __builtin_fma: a single rounding on the host and on the device.
SBLAS_NARROW_HD double sddmm_narrow_dot(const double *x, const double *y, int kp)
{
    if (kp <= 4) {
        double s = 0.0;
        for (int j = 0; j < kp; ++j) s = __builtin_fma(x[j], y[j], s);
        return s;
    }
    double s0 = 0.0, s1 = 0.0;
    s0 = __builtin_fma(x[0], y[0], s0), s0 = __builtin_fma(x[1], y[1], s0);
    s0 = __builtin_fma(x[4], y[4], s0), s0 = __builtin_fma(x[5], y[5], s0);
    s1 = __builtin_fma(x[2], y[2], s1), s1 = __builtin_fma(x[3], y[3], s1);
    s1 = __builtin_fma(x[6], y[6], s1), s1 = __builtin_fma(x[7], y[7], s1);
    return s0 + s1;
}

// the value of an entry from its sum (inside the part) or without one (outside); old is read by the caller only when beta != 0
SBLAS_NARROW_HD double sddmm_narrow_out(bool inside, double s, double alpha, double beta, double old)
{
    if (!inside) return beta == 0.0 ? 0.0 : beta * old;
    const double sres = alpha * s;
    return beta == 0.0 ? sres : __builtin_fma(beta, old, sres);
}

} // namespace sblas
