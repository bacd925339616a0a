// cheby_launch.h -- cheby.hip's launches for the other plan that smooths with the polynomial (amg.hip, one operator a
// level): the setup of one operator and the three launches of an application.  Internal C++, not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sblas {

// One matrix the polynomial works on.  units: the rows packed into four-lane records (row, beg, end, q) as the AMG
// sweep's launch packs them; dinv: n doubles, written by setup; blk: CHEBY_BLOCK_SLOTS eight-byte slots (cheby.h) with
// the table; part: krylov_cells(n) doubles, the dots' partial sums.
struct ChebyOperator {
    int64_t n = 0, units = 0;
    const void *d_units = nullptr;
    const int32_t *rowptr = nullptr, *colidx = nullptr, *dpos = nullptr;
    const double *val = nullptr;
    double *dinv = nullptr, *blk = nullptr, *part = nullptr;
};

// dinv, the row bound and the flag (the least (level << 32) | row whose diagonal is not finite and > 0, an integer
// atomicMin into *flag, which the caller has set to ~0); with `given` a NaN the estimate of `steps` steps from the start
// vector of salt seed + level, in the work vectors r, z, p, q (n doubles each, free to reuse afterwards); then the scalar
// routine and the table of `degree` entries.  Launches only.
void cheby_setup_launches(hipStream_t s, const ChebyOperator &op, unsigned long long *flag, int level, uint32_t seed, int steps, double boost,
                          double ratio, double given, int degree, double *r, double *z, double *p, double *q);
// step 0 from zero, step 0 from the guess x, step k >= 1: one launch each (cheby.hip states them)
void cheby_first_launch(hipStream_t s, const ChebyOperator &op, const double *b, double *d, double *y);
void cheby_guess_launch(hipStream_t s, const ChebyOperator &op, const double *b, const double *x, double *d, double *y);
void cheby_step_launch(hipStream_t s, const ChebyOperator &op, int k, const double *b, const double *x, double *d, double *y);

} // namespace sblas
