// gmres.h -- what gmres.hip's kernels and gmres_rule.cpp's host rule agree on: the sizes, the layout of the two device
// blocks, and the scalar step and the back substitution themselves, compiled for the host and for the device from this
// one text.  No HIP in here: GMRES_HD is empty unless the including file sets it, so gmres_rule.cpp is testable on a
// CPU box.  The cell (KRYLOV_CELL) and the width (KRYLOV_LANES) are krylov.h's.
#pragma once
#include <math.h>
#include <stdint.h>
#include "krylov.h"

#ifndef GMRES_HD
#define GMRES_HD
#endif

// The functions below are pinned bit by bit: no multiply-add may be fused, whoever includes this and wherever.
#pragma clang fp contract(off)

namespace sblas {

constexpr int GMRES_MAX_RESTART = 64;
constexpr int GMRES_DEFAULT_RESTART = 30;
constexpr int GMRES_MAX_DOTS = 65;    // columns of one multi-dot pass: v_0 .. v_m
constexpr int GMRES_DOT_GROUP = 4;    // columns whose loads are in flight together (cannot reach the bits)
constexpr int GMRES_EXTRA_VECTORS = 3; // w, u, z beside the m + 1 columns of V (ILU(0) adds the solves' temporary)

// status codes and the first five denominators are the Krylov block's (include/sblas_hip.h); restated so that this
// header needs nothing else
constexpr int GMRES_RUNNING = 0, GMRES_CONVERGED = 1, GMRES_BREAKDOWN = 2, GMRES_LIMIT = 3;
constexpr int GMRES_DENOM_GIVENS = 6; // d = sqrt(h_j^2 + eta^2) is zero or not finite
constexpr int GMRES_DENOM_BETA = 7;   // |r| of a cycle's first residual is not finite

// The scalar block: GMRES_BLOCK_SLOTS eight-byte slots.  Slots 0 - 3, 7 and 9 - 11 mean what they mean in the Krylov
// block (krylov.h); the others are GMRES's.  status, iterations, restarts, columns, which, max_iter, m and the flags
// are int64; the rest doubles.
enum GmresSlot {
    GS_STATUS = 0,
    GS_ITER = 1,     // finished Arnoldi steps
    GS_RNORM = 2,    // |g_{k}| of the recurrence, or |b - A x| as a cycle began
    GS_BNORM = 3,
    GS_ETA = 4,      // the divisor of the next normalisation: beta as a cycle begins, eta after a step
    GS_RESTARTS = 5,
    GS_COLS = 6,     // k: finished columns of the open cycle; the next step is step k
    GS_WHICH = 7,    // the denominator of a breakdown, else 0
    GS_PENDING = 8,  // 1: the k columns' correction is not in x yet.  Set by a step that finishes a column, cleared
                     //    by the close that applies it; a close acts only when this is 1
    GS_TOL = 9,      // max(rtol * |b|, atol)
    GS_MAX_ITER = 10,
    GS_ZERO_X = 11,  // b == 0: start's vector pass writes x = 0
    GS_M = 12,       // the restart length
    GS_CLOSE = 13,   // written by every close's first kernel: 1 when this close acts, and its other kernels read it
    GS_ACTIVE = 14,  // written by a step's first fold and by a cycle's first: 1 while the kernels behind it are to act
    GMRES_BLOCK_SLOTS = 16
};

// The small-matrix block, doubles: R by columns with leading dimension GMRES_MAX_RESTART, then c, s, g, y, h (the
// Hessenberg column being built) and h2 (the second pass's coefficients).
constexpr int GM_R = 0;
constexpr int GM_C = GM_R + GMRES_MAX_RESTART * GMRES_MAX_RESTART;
constexpr int GM_S = GM_C + GMRES_MAX_RESTART;
constexpr int GM_G = GM_S + GMRES_MAX_RESTART;
constexpr int GM_Y = GM_G + GMRES_MAX_RESTART + 8; // g has m + 1 entries
constexpr int GM_H = GM_Y + GMRES_MAX_RESTART;
constexpr int GM_H2 = GM_H + GMRES_MAX_RESTART + 8;
constexpr int GMRES_MATRIX_DOUBLES = GM_H2 + GMRES_MAX_RESTART + 8;

// The scalar step of Arnoldi step j, every operation rounded on its own (contraction is off from here on).
// h[0 .. j]: the new Hessenberg column after both Gram-Schmidt passes, rotated in place; eta = |w|.  c, s: the
// rotations, entries 0 .. j - 1 read, entry j written; g: entries j, j + 1 written; rcol: column j of R, j + 1 entries.
// Returns the new status.  On a breakdown (d zero or not finite) only h has changed: the columns before j stay valid.
GMRES_HD inline int gmres_step(int j, double *h, double eta, double *c, double *s, double *g, double *rcol, double tol, int64_t max_iter,
                               int64_t *iter, double *rnorm, int64_t *which)
{
    for (int i = 0; i < j; ++i) {
        const double t = c[i] * h[i] + s[i] * h[i + 1];
        h[i + 1] = (-s[i]) * h[i] + c[i] * h[i + 1];
        h[i] = t;
    }
    const double d = sqrt(h[j] * h[j] + eta * eta);
    if (d == 0.0 || !isfinite(d)) {
        *which = GMRES_DENOM_GIVENS;
        return GMRES_BREAKDOWN;
    }
    c[j] = h[j] / d;
    s[j] = eta / d;
    for (int i = 0; i < j; ++i) rcol[i] = h[i];
    rcol[j] = d;
    g[j + 1] = (-s[j]) * g[j];
    g[j] = c[j] * g[j];
    const double res = fabs(g[j + 1]);
    *rnorm = res;
    *iter = *iter + 1;
    if (res <= tol) return GMRES_CONVERGED; // a NaN never converges: the comparison is false
    if (*iter >= max_iter) return GMRES_LIMIT;
    return GMRES_RUNNING;
}

// y from R y = g over the k finished columns; R by columns with leading dimension ldr.
GMRES_HD inline void gmres_back_substitute(int k, const double *R, int ldr, const double *g, double *y)
{
    for (int i = k - 1; i >= 0; --i) {
        double t = g[i];
        for (int l = i + 1; l < k; ++l) t = t - R[(int64_t)l * ldr + i] * y[l];
        y[i] = t / R[(int64_t)i * ldr + i];
    }
}

// The first residual of a cycle (start and every restart): the test, the limit, then the breakdown.  Returns the status.
GMRES_HD inline int gmres_begin(double beta, double tol, int64_t iter, int64_t max_iter, int64_t *which)
{
    if (beta <= tol) return GMRES_CONVERGED;
    if (iter >= max_iter) return GMRES_LIMIT;
    if (!isfinite(beta)) {
        *which = GMRES_DENOM_BETA;
        return GMRES_BREAKDOWN;
    }
    return GMRES_RUNNING;
}

} // namespace sblas
