// eigsh.h -- what eigsh.hip's kernels and eigsh_rule.cpp's host rule agree on: the sizes, the layout of
// the two device blocks, and the scalar rules of the Ritz step -- the Jacobi rotation, the round-robin pairing, the update
// of a 2 x 2 block, the order of the Ritz values and the status -- compiled for the host and for the device from this one
// text, as gmres.h and cheby.h are.  No HIP in here: EIGSH_HD is empty unless the including file sets it, so
// eigsh_rule.cpp is testable on a CPU box.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef EIGSH_HD
#define EIGSH_HD
#endif

// The functions below are pinned bit by bit: no multiply-add may be fused, whoever includes this and wherever.
#pragma clang fp contract(off)

namespace sblas {

constexpr int EIGSH_MAX_NCV = 64;      // columns of a cycle: T is at most 64 x 64, V has ncv + 1 columns
constexpr int EIGSH_LD = 64;           // leading dimension of T, Y and Q in the small-matrix block
constexpr int EIGSH_DEFAULT_NCV = 20;  // ncv = min(max(2 k + 1, 20), 64, n - 1)
constexpr int EIGSH_MAX_SWEEPS = 24;   // the cap on Jacobi sweeps; a sweep without a rotation ends the loop before it
constexpr int EIGSH_RITZ_THREADS = 256;
constexpr int EIGSH_ROTATE_THREADS = 256; // rows of V a workgroup of the rotation takes, one a lane

constexpr int EIGSH_LA = 0, EIGSH_SA = 1, EIGSH_LM = 2;
constexpr int EIGSH_RUNNING = 0, EIGSH_CONVERGED = 1, EIGSH_BREAKDOWN = 2, EIGSH_LIMIT = 3; // the Krylov block's codes
// what a breakdown names (ES_WHICH)
constexpr int EIGSH_DENOM_V0 = 1;       // |v0| is zero or not finite
constexpr int EIGSH_DENOM_BETA = 2;     // beta of a step is not finite
constexpr int EIGSH_DENOM_T = 3;        // T holds a value that is not finite
constexpr int EIGSH_DENOM_INVARIANT = 4; // beta == 0 with fewer than k columns: ES_MM names the count

// The scalar block: eight-byte slots.  status, the counts and the flags are int64; beta, rtol and atol doubles.
enum EigshSlot {
    ES_STATUS = 0,
    ES_RESTARTS = 1,  // Ritz steps taken
    ES_MATVECS = 2,   // finished Lanczos steps
    ES_COLS = 3,      // finished columns of T in the open cycle; step j acts when this is j
    ES_BETA = 4,      // |w| of the last finished step (|v0| behind start's first fold)
    ES_WHICH = 5,     // EIGSH_DENOM_* of a breakdown, else 0
    ES_ACT = 6,       // raised by a Ritz step that acts, read by the rotation behind it, cleared by the next Ritz kernel
    ES_ACTIVE = 7,    // written by a step's first fold: 1 while the kernels behind it are to act
    ES_RTOL = 8,
    ES_ATOL = 9,
    ES_MAX_RESTARTS = 10,
    ES_CONVERGED = 11, // how many of the first k estimates met the test at the last Ritz step
    ES_INVARIANT = 12, // a step met beta == 0: no further step acts, the Ritz step ends the solve
    ES_MM = 13,        // the column count of the last Ritz step: what the rotation reads
    ES_KK = 14,        // min(keep, mm): the columns the rotation writes
    EIGSH_BLOCK_SLOTS = 16
};

// The small-matrix block, doubles.  T and Y by columns with leading dimension EIGSH_LD (T is kept symmetric, so by rows
// as well), theta and the residual estimates in the order of `which`, Q = the kept columns of Y in that order (mm x kk,
// by columns), h and c the coefficients of the two Gram-Schmidt passes.
constexpr int EM_T = 0;
constexpr int EM_Y = EM_T + EIGSH_LD * EIGSH_MAX_NCV;
constexpr int EM_THETA = EM_Y + EIGSH_LD * EIGSH_MAX_NCV;
constexpr int EM_RHO = EM_THETA + EIGSH_MAX_NCV;
constexpr int EM_Q = EM_RHO + EIGSH_MAX_NCV;
constexpr int EM_H = EM_Q + EIGSH_LD * EIGSH_MAX_NCV;
constexpr int EM_C = EM_H + EIGSH_MAX_NCV + 8;
constexpr int EIGSH_MATRIX_DOUBLES = EM_C + EIGSH_MAX_NCV + 8;

inline bool eigsh_which_ok(int which) { return which == EIGSH_LA || which == EIGSH_SA || which == EIGSH_LM; }
inline int eigsh_default_ncv(int64_t n, int k)
{
    int64_t ncv = 2 * (int64_t)k + 1 > EIGSH_DEFAULT_NCV ? 2 * (int64_t)k + 1 : EIGSH_DEFAULT_NCV;
    if (ncv > EIGSH_MAX_NCV) ncv = EIGSH_MAX_NCV;
    if (ncv > n - 1) ncv = n - 1;
    return (int)ncv;
}
inline int eigsh_default_keep(int k, int ncv) { return k + (ncv - k) / 2; }
// 1 <= k < ncv <= min(64, n - 1) and k <= keep <= ncv - 1
inline bool eigsh_sizes_ok(int64_t n, int k, int ncv, int keep)
{
    return k >= 1 && k < ncv && ncv <= EIGSH_MAX_NCV && ncv < n && keep >= k && keep <= ncv - 1;
}

// Pair i (0 <= i < M / 2) of round r (0 <= r < M - 1) among M players, M even: the circle method with player M - 1
// fixed.  Every two players meet once in M - 1 rounds, and a round's pairs are disjoint.  p < q.
EIGSH_HD inline void eigsh_pair(int M, int r, int i, int *p, int *q)
{
    const int ring = M - 1;
    int a = (r + i) % ring, b = i == 0 ? ring : (r - i + ring) % ring;
    *p = a < b ? a : b, *q = a < b ? b : a;
}

// The rotation that annihilates a_pq: (c, s) with t = s / c the smaller root, and the two new diagonal entries.  False:
// the off-diagonal is negligible beside both diagonal entries (or zero) and the pair is skipped, c = 1, s = 0.  Either
// way the caller stores 0 for a_pq.  |tau| >= 2^500 (tau * tau would overflow) takes t = 1 / (2 tau).
EIGSH_HD inline bool eigsh_rotation(double app, double aqq, double apq, double *c, double *s, double *dpp, double *dqq)
{
    const double g = fabs(apq), fp = fabs(app), fq = fabs(aqq);
    if (g == 0.0 || (fp + g == fp && fq + g == fq)) {
        *c = 1.0, *s = 0.0, *dpp = app, *dqq = aqq;
        return false;
    }
    const double tau = (aqq - app) / (2.0 * apq), at = fabs(tau);
    double t;
    if (at >= 0x1p500) {
        t = 0.5 / tau;
    } else {
        const double root = sqrt(1.0 + tau * tau);
        t = 1.0 / (at + root);
        if (tau < 0.0) t = -t;
    }
    const double cc = 1.0 / sqrt(1.0 + t * t), d = t * apq;
    *c = cc, *s = t * cc, *dpp = app - d, *dqq = aqq + d;
    return true;
}

// x <- x J over the columns (xp, xq) of one row: J = [c s; -s c]
EIGSH_HD inline void eigsh_rotate_pair(double c, double s, double *xp, double *xq)
{
    const double a = *xp, b = *xq;
    *xp = c * a - s * b;
    *xq = s * a + c * b;
}

// The 2 x 2 block of T at rows (p1, q1) and columns (p2, q2) of two different pairs, B <- J1^T B J2.  upper (the row
// pair's index is below the column pair's): the column rotation first, then the row rotation; else the other way round,
// which is the upper block's arithmetic transposed -- so a symmetric T stays symmetric to the bit.
EIGSH_HD inline void eigsh_block(bool upper, double c1, double s1, double c2, double s2, double *bpp, double *bpq, double *bqp, double *bqq)
{
    if (upper) {
        eigsh_rotate_pair(c2, s2, bpp, bpq), eigsh_rotate_pair(c2, s2, bqp, bqq);
        eigsh_rotate_pair(c1, s1, bpp, bqp), eigsh_rotate_pair(c1, s1, bpq, bqq);
    } else {
        eigsh_rotate_pair(c1, s1, bpp, bqp), eigsh_rotate_pair(c1, s1, bpq, bqq);
        eigsh_rotate_pair(c2, s2, bpp, bpq), eigsh_rotate_pair(c2, s2, bqp, bqq);
    }
}

// Does Ritz value a (at index ia) come before b (at ib)?  LA: descending; SA: ascending; LM: descending |theta|; ties by
// index.  The values are finite.
EIGSH_HD inline bool eigsh_before(int which, double a, int ia, double b, int ib)
{
    if (which == EIGSH_LM) a = fabs(a), b = fabs(b);
    if (a == b) return ia < ib;
    return which == EIGSH_SA ? a < b : a > b;
}

// does the estimate rho meet the test for theta?  A NaN never does.
EIGSH_HD inline bool eigsh_met(double rho, double theta, double rtol, double atol)
{
    const double rel = rtol * fabs(theta), tol = rel >= atol ? rel : atol;
    return rho <= tol;
}

// The status behind a Ritz step over mm columns: `met` of the first k estimates met the test, `restarts` counts this step.
EIGSH_HD inline int eigsh_decide(int mm, int k, int met, bool invariant, int64_t restarts, int64_t max_restarts, int64_t *which)
{
    if (mm < k) { // only an invariant subspace ends a cycle this short
        *which = EIGSH_DENOM_INVARIANT;
        return EIGSH_BREAKDOWN;
    }
    if (met == k || invariant) return EIGSH_CONVERGED;
    if (restarts >= max_restarts) return EIGSH_LIMIT;
    return EIGSH_RUNNING;
}

// The scalar part of a step's last fold, behind beta = sqrt((w, w)): T's column j from h, the count, and what beta
// means.  Returns whether v_{j+1} = w / beta is to be formed.
EIGSH_HD inline bool eigsh_step(int j, const double *h, double beta, double *T, double *blk)
{
    int64_t *ib = reinterpret_cast<int64_t *>(blk);
    for (int i = 0; i <= j; ++i) T[(int64_t)j * EIGSH_LD + i] = h[i], T[(int64_t)i * EIGSH_LD + j] = h[i];
    blk[ES_BETA] = beta;
    ib[ES_MATVECS] = ib[ES_MATVECS] + 1;
    if (!isfinite(beta)) {
        ib[ES_STATUS] = EIGSH_BREAKDOWN, ib[ES_WHICH] = EIGSH_DENOM_BETA, ib[ES_ACTIVE] = 0;
        return false;
    }
    ib[ES_COLS] = j + 1;
    if (beta == 0.0) { // an invariant subspace: the cycle ends at j + 1 columns
        ib[ES_INVARIANT] = 1, ib[ES_ACTIVE] = 0;
        return false;
    }
    return true;
}

} // namespace sblas
