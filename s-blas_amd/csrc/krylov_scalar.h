// krylov_scalar.h -- the scalar step of PCG and BiCGStab, once: what lane 0 of a fold does with a pass's folded sums in
// one device scalar block (alpha, beta, omega, |r|, the stopping test, the count, the status word).  krylov.hip runs it
// on its one block, krylov_multi.hip on column j's block, and krylov_multi_rule.cpp compiles the same text for the
// host (sblas_krylov_scalar_step_ref), so the three cannot drift apart.  Quotients, one product and square roots
// only: nothing in here can be contracted.  No HIP in here beyond the two qualifiers.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/sblas_hip.h"
#include "krylov.h"

#if defined(__HIPCC__)
#define SBLAS_SCALAR_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define SBLAS_SCALAR_FN inline
#endif

namespace sblas {

// fold ops: what the step does with the folded sums d[0 .. nd - 1] (SBLAS_KRYLOV_STEP_* in sblas_hip_krylov_multi.h)
enum {
    FOLD_OUT = 0,                                       // out[k] = d[k]: the fold's own business, not a step
    FOLD_START_B = SBLAS_KRYLOV_STEP_START_B,           // |b|, the tolerance, and the block's first state (flag: BiCGStab)
    FOLD_START_R = SBLAS_KRYLOV_STEP_START_R,           // |r0| and the test at iteration 0; rho = d[nd - 1]
    FOLD_RHO0 = SBLAS_KRYLOV_STEP_RHO0,                 // rho = d[0]                                     (PCG with an applied M^-1: (r0, z0))
    FOLD_PCG_ALPHA = SBLAS_KRYLOV_STEP_PCG_ALPHA,       // alpha = rho / (p, q)
    FOLD_PCG_RES = SBLAS_KRYLOV_STEP_PCG_RES,           // |r|, count, test; flag: then beta = d[nd - 1] / rho
    FOLD_PCG_BETA = SBLAS_KRYLOV_STEP_PCG_BETA,         // beta = d[0] / rho                              (PCG with an applied M^-1)
    FOLD_BICG_ALPHA = SBLAS_KRYLOV_STEP_BICG_ALPHA,     // alpha = rho / (r^, v)
    FOLD_BICG_OMEGA = SBLAS_KRYLOV_STEP_BICG_OMEGA,     // omega = (t, s) / (t, t); d[2] = (s, s) for the half step that already meets the test
    FOLD_BICG_RES = SBLAS_KRYLOV_STEP_BICG_RES          // |r|, count, test, beta = ((r^, r) / rho) * (alpha / omega)
};

SBLAS_SCALAR_FN bool bad_denominator(double d) { return d == 0.0 || !isfinite(d); }

SBLAS_SCALAR_FN void break_down(double *blk, long long which)
{
    long long *ib = reinterpret_cast<long long *>(blk);
    ib[KS_STATUS] = SBLAS_KRYLOV_BREAKDOWN, ib[KS_WHICH] = which;
}

// |r|, the count and the test; true when the recurrence goes on
SBLAS_SCALAR_FN bool residual_step(double *blk, double rr, bool count)
{
    long long *ib = reinterpret_cast<long long *>(blk);
    const double rnorm = sqrt(rr);
    blk[KS_RNORM] = rnorm;
    if (count) ib[KS_ITER] = ib[KS_ITER] + 1;
    if (rnorm <= blk[KS_TOL]) ib[KS_STATUS] = SBLAS_KRYLOV_CONVERGED;
    else if (ib[KS_ITER] >= ib[KS_MAX_ITER]) ib[KS_STATUS] = SBLAS_KRYLOV_LIMIT;
    else return true;
    return false;
}

// One step `op` (not FOLD_OUT) on the block blk with the folded sums d[0 .. nd - 1].  rtol, atol and max_iter are read
// by FOLD_START_B alone.
SBLAS_SCALAR_FN void krylov_scalar_step(int op, int nd, int flag, const double *d, double *blk, double rtol, double atol, long long max_iter)
{
    long long *ib = reinterpret_cast<long long *>(blk);
    if (op == FOLD_START_B) {
        const double bnorm = sqrt(d[0]), t = rtol * bnorm;
        // every slot by its own type: a slot is never read as the other one
        blk[KS_RNORM] = 0.0, blk[KS_ALPHA] = 0.0, blk[KS_BETA] = 0.0, blk[KS_RHO] = 0.0, blk[KS_OMEGA] = flag ? 1.0 : 0.0;
        blk[KS_BNORM] = bnorm, blk[KS_TOL] = t >= atol ? t : atol;
        ib[KS_ITER] = 0, ib[KS_WHICH] = 0, ib[KS_MAX_ITER] = max_iter;
        const bool zero = d[0] == 0.0; // b == 0: x = 0, converged at iteration 0, and nothing is divided
        ib[KS_ZERO_X] = zero, ib[KS_STATUS] = zero ? SBLAS_KRYLOV_CONVERGED : SBLAS_KRYLOV_RUNNING;
        return;
    }
    if (ib[KS_STATUS] != SBLAS_KRYLOV_RUNNING) return; // frozen: the scalars stay what they were
    const double rho = blk[KS_RHO];
    switch (op) {
    case FOLD_START_R:
        blk[KS_RHO] = d[nd - 1];
        residual_step(blk, d[0], false);
        break;
    case FOLD_RHO0: blk[KS_RHO] = d[0]; break;
    case FOLD_PCG_ALPHA:
    case FOLD_BICG_ALPHA:
        if (bad_denominator(d[0])) break_down(blk, op == FOLD_PCG_ALPHA ? SBLAS_KRYLOV_DENOM_PQ : SBLAS_KRYLOV_DENOM_RV);
        else blk[KS_ALPHA] = rho / d[0];
        break;
    case FOLD_PCG_RES:
        if (!residual_step(blk, d[0], true) || !flag) break;
        [[fallthrough]];
    case FOLD_PCG_BETA: {
        const double rho_new = d[op == FOLD_PCG_RES ? nd - 1 : 0];
        if (bad_denominator(rho)) break_down(blk, SBLAS_KRYLOV_DENOM_RHO);
        else blk[KS_BETA] = rho_new / rho, blk[KS_RHO] = rho_new;
        break;
    }
    case FOLD_BICG_OMEGA:
        // t = 0 because s already meets the test (A s^ of a vanished s): the half step is the answer, omega = 0 takes it
        if (d[1] == 0.0 && sqrt(d[2]) <= blk[KS_TOL]) blk[KS_OMEGA] = 0.0;
        else if (bad_denominator(d[1])) break_down(blk, SBLAS_KRYLOV_DENOM_TT);
        else blk[KS_OMEGA] = d[0] / d[1];
        break;
    case FOLD_BICG_RES:
        if (!residual_step(blk, d[0], true)) break;
        if (bad_denominator(rho)) break_down(blk, SBLAS_KRYLOV_DENOM_RHO);
        else if (bad_denominator(blk[KS_OMEGA])) break_down(blk, SBLAS_KRYLOV_DENOM_OMEGA);
        else blk[KS_BETA] = (d[1] / rho) * (blk[KS_ALPHA] / blk[KS_OMEGA]), blk[KS_RHO] = d[1];
        break;
    default: break;
    }
}

} // namespace sblas
