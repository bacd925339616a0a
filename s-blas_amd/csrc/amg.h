// amg.h -- what amg.hip's kernels and amg_rule.cpp's host rule agree on: the lane groups of a row sweep,
// the defaults, the order of a V-cycle as ONE walk both sides instantiate, and the host rule's internal interface.  No
// HIP in here: amg_rule.cpp is testable on a CPU box.
#pragma once
#include <math.h>
#include <stdint.h>
#include <vector>
#include "sptrsv.h"

namespace sblas {

// A row of p stored entries is summed by the solves' G(p) lanes (sptrsv_group_shift): 4 lanes up to AMG_G4_MAX, 16 up to
// AMG_G16_MAX, a whole wave beyond.
constexpr int64_t AMG_G4_MAX = SPTRSV_G4_MAX;
constexpr int64_t AMG_G16_MAX = SPTRSV_G16_MAX;
constexpr int AMG_THREADS = 256; // a workgroup of every AMG kernel: four waves
constexpr int64_t AMG_COARSE_MAX = 64;
constexpr int AMG_MAX_LEVELS = 20;
constexpr int AMG_LEVEL_CAP = 64; // max_levels is at most this
constexpr int AMG_NU = 1;
constexpr int AMG_COARSE_SWEEPS = 8;
constexpr int AMG_SWEEP_CAP = 1 << 20; // nu and coarse_sweeps are at most this: launch counts stay far inside int64

// The vectors of one level.  b: the right-hand side (level 0: the caller's r); x[0], x[1]: the two iterates a sweep
// ping-pongs between (other rows gather x while y is written); res: the residual that is restricted.  Level 0's last
// write must land in the caller's z, so z is whichever of x[0] / x[1] the parity of the level's writes selects
// (amg_first_buffer).
//
// One V(nu, nu) cycle from a zero guess, as calls on `ops` -- the device enqueues a launch for each, the host
// reference computes it, the launch counter counts it.  `cur` is the index of the buffer that holds the level's iterate.
//   first(l, dst)          x[dst] = wd o b                        (the first sweep from zero)
//   sweep(l, src, dst)     x[dst] = x[src] + wd o (b - A x[src])
//   residual(l, src)       res = b - A x[src]
//   restrict_to(l)         b of level l + 1 = sums of res over the aggregates of level l
//   prolong(l, dst)        x[dst] of level l += scale * (the iterate of level l + 1)[agg]
// The iterate of level l ends in x[amg_last_buffer(...)], which both sides compute the same way.
//
// With the Chebyshev smoother (degree >= 1, 0 means the sweeps above) every one of the nu smoothings is one
// polynomial of `degree` launches in D^-1 A (wd holds 1 / a_ii, d is the level's direction vector, the table the level's
// own): the pre-smoothing's first goes from zero, every other one from the current iterate; the coarsest level runs one
// polynomial of degree coarse_sweeps from zero.
//   poly_first(l, dst)          d = c2_0 (wd o b), x[dst] = d
//   poly_guess(l, src, dst)     d = c2_0 (wd o (b - A x[src])), x[dst] = x[src] + d
//   poly_step(l, k, src, dst)   d = c1_k d + c2_k (wd o (b - A x[src])), x[dst] = x[src] + d
inline int amg_level_writes(int level, int levels, int nu, int coarse_sweeps, int degree = 0)
{
    return level + 1 == levels ? coarse_sweeps : 2 * nu * (degree > 0 ? degree : 1);
}
// the buffer the first write goes to, so that the last one lands in buffer 1
inline int amg_first_buffer(int level, int levels, int nu, int coarse_sweeps, int degree = 0)
{
    return amg_level_writes(level, levels, nu, coarse_sweeps, degree) % 2 ? 1 : 0;
}
constexpr int AMG_RESULT_BUFFER = 1; // every level's iterate ends here (level 0: the caller's z)

template <typename Ops> void amg_cycle(int levels, int nu, int coarse_sweeps, Ops &ops, int level = 0, int degree = 0)
{
    if (levels <= 0) return;
    int cur = amg_first_buffer(level, levels, nu, coarse_sweeps, degree);
    // one smoothing of the iterate in `cur` (from zero: into it): a sweep, or a polynomial of `steps` launches
    const auto smooth = [&](bool from_zero, int steps) {
        if (degree == 0) {
            if (from_zero) ops.first(level, cur);
            else ops.sweep(level, cur, cur ^ 1), cur ^= 1;
            return;
        }
        if (from_zero) ops.poly_first(level, cur);
        else ops.poly_guess(level, cur, cur ^ 1), cur ^= 1;
        for (int k = 1; k < steps; ++k) ops.poly_step(level, k, cur, cur ^ 1), cur ^= 1;
    };
    if (level + 1 == levels) {
        if (degree > 0) return smooth(true, coarse_sweeps);
        smooth(true, 1);
        for (int k = 1; k < coarse_sweeps; ++k) smooth(false, 1);
        return;
    }
    smooth(true, degree);
    for (int k = 1; k < nu; ++k) smooth(false, degree);
    ops.residual(level, cur);
    ops.restrict_to(level);
    amg_cycle(levels, nu, coarse_sweeps, ops, level + 1, degree);
    ops.prolong(level, cur);
    for (int k = 0; k < nu; ++k) smooth(false, degree);
}

// launches of one cycle: every call of the walk is one launch
struct AmgCount {
    int64_t n = 0;
    void first(int, int) { ++n; }
    void sweep(int, int, int) { ++n; }
    void poly_first(int, int) { ++n; }
    void poly_guess(int, int, int) { ++n; }
    void poly_step(int, int, int, int) { ++n; }
    void residual(int, int) { ++n; }
    void restrict_to(int) { ++n; }
    void prolong(int, int) { ++n; }
};

inline bool amg_cycle_args_ok(int levels, int nu, int coarse_sweeps)
{
    return levels >= 0 && levels <= AMG_LEVEL_CAP && nu >= 1 && nu <= AMG_SWEEP_CAP && coarse_sweeps >= 1 && coarse_sweeps <= AMG_SWEEP_CAP;
}
// with the Chebyshev smoother the coarsest level's polynomial has coarse_sweeps entries in its table
inline bool amg_cheb_args_ok(int degree, int coarse_sweeps) { return degree >= 1 && degree <= 64 && coarse_sweeps <= 64; }
inline bool amg_theta_ok(double theta) { return theta >= 0.0 && theta <= 1.0; } // a NaN fails both

// Smoothed aggregation.  The coarsening guard: a level of n rows whose aggregation leaves n_next is kept
// only when it reduces n at all (the plain plan's rule) and n_next <= (1 - min_reduction) * n, the product rounded once.
constexpr double AMG_PROLONG_OMEGA = 2.0 / 3.0;        // 4 / (3 rho) with rho(D^-1 A) taken as 2: no eigenvalue estimate
constexpr double AMG_SMOOTHED_MIN_REDUCTION = 0.2;     // the Python layer's default for a smoothed plan
inline bool amg_min_reduction_ok(double m) { return m >= 0.0 && m < 1.0; } // a NaN fails both
inline bool amg_prolong_omega_ok(double w) { return w > 0.0 && w <= 1.79769313486231570815e308; } // finite, > 0; a NaN fails
inline bool amg_keep_level(int64_t n, int64_t n_next, double min_reduction)
{
    const double bound = (1.0 - min_reduction) * (double)n;
    return n_next < n && (double)n_next <= bound;
}
enum { AMG_RESTRICT = 0, AMG_PROLONG = 1 }; // modes of the transfer row product

// The row sum in the solves' pinned order, on the host (the references of amg_rule.cpp and cheby_rule.cpp): G(p) lanes,
// lane l the entries l, l + G, ... with one fused multiply-add each from +0, then the butterfly l ^ 1, l ^ 2, ... as
// written; lane 0 holds the result.  fma() by name and additions only: nothing here can be contracted.
inline double amg_row_sum(const int32_t *colidx, const double *val, int64_t beg, int64_t end, const double *x)
{
    const int G = 1 << sptrsv_group_shift(end - beg);
    double v[64], w[64];
    for (int l = 0; l < G; ++l) {
        double s = 0.0;
        for (int64_t e = beg + l; e < end; e += G) s = fma(val[e], x[colidx[e]], s);
        v[l] = s;
    }
    for (int m = 1; m < G; m <<= 1) {
        for (int l = 0; l < G; ++l) w[l] = v[l] + v[l ^ m];
        for (int l = 0; l < G; ++l) v[l] = w[l];
    }
    return v[0];
}

// One level's aggregation on host arrays (sblas_amg_aggregate without the argument checks): agg (n), aggptr (n_agg + 1,
// resized here), members (n) -> n_agg.  val may be null (structure only).
int64_t amg_aggregate(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, double theta, uint32_t seed,
                      uint32_t level, int32_t *agg, std::vector<int32_t> &aggptr, int32_t *members);

// The bound of the strength test, theta * max_{k != i} |a_ik| for every row (val != null, theta > 0): amg_aggregate's.
void amg_strength_bounds(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, double theta, std::vector<double> &bound);

// The same rule in synchronous rounds (sblas_amg_roots_rounds_ref without the argument checks): root (n
// bytes, 1 = root) -> the rounds that decided a vertex.
int64_t amg_roots_rounds(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, double theta, uint32_t seed, uint32_t level,
                         unsigned char *root);

} // namespace sblas
