// cheby.h -- what cheby.hip's kernels and cheby_rule.cpp's host rule agree on: the sizes, the layout of
// the device scalar block, and the scalar routine itself -- the tridiagonal of the Lanczos recurrence, its largest Ritz
// value by Sturm bisection, the interval and the coefficient table of the polynomial -- compiled for the host and for the
// device (one lane) from this one text, as gmres.h is.  No HIP in here: CHEBY_HD is empty unless the including file
// sets it, so cheby_rule.cpp is testable on a CPU box.  The routine indexes no local array: its work arrays are the
// caller's (the device hands it slots of the scalar block), so the device side needs no scratch.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#ifndef CHEBY_HD
#define CHEBY_HD
#endif

// The functions below are pinned bit by bit: no multiply-add may be fused, whoever includes this and wherever.
#pragma clang fp contract(off)

namespace sblas {

constexpr int CHEBY_THREADS = 256;    // a workgroup of the step kernel: four waves, as the AMG sweep's
constexpr int CHEBY_MAX_DEGREE = 64;
constexpr int CHEBY_MAX_STEPS = 64;   // steps of the eigenvalue estimate
constexpr int CHEBY_DEFAULT_DEGREE = 4;
constexpr int CHEBY_DEFAULT_STEPS = 10;
constexpr double CHEBY_DEFAULT_BOOST = 1.1;
constexpr double CHEBY_DEFAULT_RATIO = 30.0;
constexpr int CHEBY_BISECTIONS = 64;

constexpr int CHEBY_RUNNING = 0, CHEBY_STOPPED = 1;

// The scalar block: eight-byte slots.  status and m are int64; flag and g's slot are written by integer atomics (g is a
// maximum of positive doubles, which order as their bit patterns do); the rest are doubles.
enum ChebySlot {
    CS_STATUS = 0, // CHEBY_RUNNING / CHEBY_STOPPED: the freeze of the estimate's batch
    CS_M = 1,      // finished Lanczos steps: alpha_0 .. alpha_{m-1} and beta_0 .. beta_{m-2} are valid
    CS_RHO = 2,    // (r, z)
    CS_ALPHA = 3,  // the current step's
    CS_BETA = 4,
    CS_FLAG = 5,   // the least row whose diagonal is not finite and > 0, or ~0
    CS_G = 6,      // the row bound max_i sum_e |a_ie| / a_ii
    CS_RITZ = 7,
    CS_LMAX = 8,
    CS_LMIN = 9,
    CS_ALPHAS = 16,
    CS_BETAS = CS_ALPHAS + CHEBY_MAX_STEPS,
    CS_T = CS_BETAS + CHEBY_MAX_STEPS,  // the tridiagonal's diagonal, the routine's work array
    CS_E2 = CS_T + CHEBY_MAX_STEPS,     // its squared off-diagonal
    CS_TABLE = CS_E2 + CHEBY_MAX_STEPS, // (c1_k, c2_k) for k = 0 .. degree - 1
    CHEBY_BLOCK_SLOTS = CS_TABLE + 2 * CHEBY_MAX_DEGREE
};

inline bool cheby_degree_ok(int degree) { return degree >= 1 && degree <= CHEBY_MAX_DEGREE; }
inline bool cheby_steps_ok(int steps) { return steps >= 1 && steps <= CHEBY_MAX_STEPS; }
inline bool cheby_boost_ok(double boost) { return boost >= 1.0 && boost <= DBL_MAX; } // finite, >= 1; a NaN fails
inline bool cheby_ratio_ok(double ratio) { return ratio > 1.0 && ratio <= DBL_MAX; }  // finite, > 1; a NaN fails
inline bool cheby_lambda_ok(double lambda) { return lambda > 0.0 && lambda <= DBL_MAX; } // a caller-given lambda_max

// a scalar of the recurrence goes on only when it is finite and > 0 (a NaN fails the comparison)
CHEBY_HD inline bool cheby_positive(double v) { return v > 0.0 && v <= DBL_MAX; }

// b0[i] from the colouring's priority hash h: (2 h + 1) 2^-32 - 1, exact in a double, in (-1, 1), never 0
CHEBY_HD inline double cheby_start_value(uint32_t h) { return (2.0 * (double)h + 1.0) * 0x1p-32 - 1.0; }

// T of m finished steps: t_0 = 1 / alpha_0, t_j = 1 / alpha_j + beta_{j-1} / alpha_{j-1}, e2_j = beta_j / (alpha_j alpha_j)
// for j < m - 1.
CHEBY_HD inline void cheby_tridiagonal(int m, const double *alpha, const double *beta, double *t, double *e2)
{
    for (int j = 0; j < m; ++j) {
        const double inv = 1.0 / alpha[j];
        if (j == 0) {
            t[j] = inv;
        } else {
            const double carry = beta[j - 1] / alpha[j - 1];
            t[j] = inv + carry;
        }
        if (j < m - 1) {
            const double aa = alpha[j] * alpha[j];
            e2[j] = beta[j] / aa;
        }
    }
}

// the number of eigenvalues of T below x: the negative terms of the Sturm sequence, an exact zero taken as -DBL_MIN
CHEBY_HD inline int cheby_sturm_count(int m, const double *t, const double *e2, double x)
{
    int count = 0;
    double q = 0.0;
    for (int j = 0; j < m; ++j) {
        const double shifted = t[j] - x;
        if (j == 0) {
            q = shifted;
        } else {
            const double ratio = e2[j - 1] / q;
            q = shifted - ratio;
        }
        if (q == 0.0) q = -DBL_MIN;
        if (q < 0.0) ++count;
    }
    return count;
}

// The largest eigenvalue of T (m >= 1) by bisection between max_j t_j and the Gershgorin bound: the upper end.
CHEBY_HD inline double cheby_ritz(int m, const double *t, const double *e2)
{
    double lo = t[0], hi = 0.0;
    for (int j = 0; j < m; ++j) {
        if (t[j] > lo) lo = t[j];
        const double left = j > 0 ? sqrt(e2[j - 1]) : 0.0, right = j < m - 1 ? sqrt(e2[j]) : 0.0;
        const double bound = (t[j] + left) + right;
        if (j == 0 || bound > hi) hi = bound;
    }
    for (int it = 0; it < CHEBY_BISECTIONS; ++it) {
        const double half = (hi - lo) / 2.0, mid = lo + half;
        if (mid <= lo || mid >= hi) break;
        if (cheby_sturm_count(m, t, e2, mid) == m) hi = mid;
        else lo = mid;
    }
    return hi;
}

// lambda_max = min(boost * Ritz, g) after m >= 1 steps, g alone after none
CHEBY_HD inline double cheby_lambda_max(int64_t m, double ritz, double g, double boost)
{
    if (m < 1) return g;
    const double boosted = boost * ritz;
    return boosted < g ? boosted : g;
}

// (c1_k, c2_k) for k = 0 .. degree - 1 on [lambda_min, lambda_max]
CHEBY_HD inline void cheby_coefficients(double lambda_max, double lambda_min, int degree, double *table)
{
    const double theta = (lambda_max + lambda_min) / 2.0, delta = (lambda_max - lambda_min) / 2.0, sigma = theta / delta;
    double rho = 1.0 / sigma;
    table[0] = 0.0, table[1] = 1.0 / theta;
    for (int k = 1; k < degree; ++k) {
        const double next = 1.0 / (2.0 * sigma - rho);
        table[2 * k] = next * rho;
        table[2 * k + 1] = (2.0 * next) / delta;
        rho = next;
    }
}

// The whole scalar step behind the recurrence: from (m, alpha, beta, g) or a caller-given lambda_max (not a NaN) to the
// Ritz value, the interval and the table.  t, e2: work arrays of CHEBY_MAX_STEPS doubles.  out: ritz, lambda_max, lambda_min.
CHEBY_HD inline void cheby_finish(int64_t m, const double *alpha, const double *beta, double g, double boost, double ratio, double given,
                                  int degree, double *t, double *e2, double *out, double *table)
{
    double ritz = 0.0, lambda_max = given;
    if (given != given) {
        if (m >= 1) {
            cheby_tridiagonal((int)m, alpha, beta, t, e2);
            ritz = cheby_ritz((int)m, t, e2);
        }
        lambda_max = cheby_lambda_max(m, ritz, g, boost);
    }
    const double lambda_min = lambda_max / ratio;
    out[0] = ritz, out[1] = lambda_max, out[2] = lambda_min;
    cheby_coefficients(lambda_max, lambda_min, degree, table);
}

// the buffer a degree-`degree` application writes first so that its last write lands in the result (buffer 1)
inline int cheby_first_buffer(int degree) { return degree % 2 ? 1 : 0; }

} // namespace sblas
