// gmres_rule.cpp -- the host rule of restarted GMRES (gmres.hip): the limits, the scalar step and the back substitution
// restated through the very functions the device compiles (gmres.h), and the launch counts of a step, a close and a
// restart.  Pure functions of host arrays; no GPU call in this file, so it is testable on a CPU box (and under a host
// sanitizer).
#include <stdint.h>
#include "../../include/sblas_hip.h"

#pragma clang fp contract(off) // ahead of gmres.h: every product and every sum of its functions is rounded on its own

#include "gmres.h"
#include "precond_rule.h"

static_assert(SBLAS_GMRES_DENOM_GIVENS == sblas::GMRES_DENOM_GIVENS && SBLAS_GMRES_DENOM_BETA == sblas::GMRES_DENOM_BETA, "gmres.h restates them");
static_assert(SBLAS_KRYLOV_RUNNING == sblas::GMRES_RUNNING && SBLAS_KRYLOV_CONVERGED == sblas::GMRES_CONVERGED &&
                  SBLAS_KRYLOV_BREAKDOWN == sblas::GMRES_BREAKDOWN && SBLAS_KRYLOV_LIMIT == sblas::GMRES_LIMIT,
              "gmres.h restates them");
static_assert(SBLAS_GMRES_MAX_RESTART == sblas::GMRES_MAX_RESTART, "the header's limit is gmres.h's");

extern "C" {

int sblas_gmres_limits(int64_t out[8])
{
    using namespace sblas;
    if (!out) return SBLAS_E_INVALID;
    out[0] = GMRES_MAX_RESTART, out[1] = GMRES_DEFAULT_RESTART, out[2] = GMRES_MAX_DOTS;
    out[3] = 1, out[4] = 1 + GMRES_EXTRA_VECTORS; // work vectors = out[3] * m + out[4] (ILU(0): one more)
    out[5] = GMRES_BLOCK_SLOTS * 8, out[6] = GMRES_MATRIX_DOUBLES * 8, out[7] = GMRES_DOT_GROUP;
    return SBLAS_OK;
}

int sblas_gmres_step_ref(int j, double *h, double eta, double *c, double *s, double *g, double *rcol, double tol, int64_t max_iter,
                         int64_t *iterations, double *rnorm, int64_t *which)
{
    if (j < 0 || j >= sblas::GMRES_MAX_RESTART || !h || !c || !s || !g || !rcol || !iterations || !rnorm || !which) return -1;
    return sblas::gmres_step(j, h, eta, c, s, g, rcol, tol, max_iter, iterations, rnorm, which);
}

int sblas_gmres_solve_ref(int k, const double *R, int ldr, const double *g, double *y)
{
    if (k < 0 || k > sblas::GMRES_MAX_RESTART || ldr < k) return SBLAS_E_INVALID;
    if (k > 0 && (!R || !g || !y)) return SBLAS_E_INVALID;
    sblas::gmres_back_substitute(k, R, ldr, g, y);
    return SBLAS_OK;
}

int64_t sblas_gmres_launches(int m, int precond, const int64_t *lower_info, const int64_t *upper_info, int64_t out[4])
{
    if (m < 1 || m > sblas::GMRES_MAX_RESTART || !out) return -1;
    const int64_t apply = sblas::precond_launches(precond, lower_info, upper_info); // launches of one M^-1
    if (apply < 0) return -1;
    // step (the same for every j: the kernels read j from the block): [M^-1;] SpMV; multi-dot, fold; projection;
    // multi-dot, fold; projection with (w, w); fold and scalar step; normalisation
    out[0] = 9 + apply;
    out[1] = 3 + apply; // close: back substitution; combination; [M^-1;] x update
    out[2] = 4;         // restart: SpMV; residual with (r, r); fold and test; normalisation
    out[3] = 6;         // start: (b, b), fold; SpMV; residual with (r, r); fold and test; normalisation
    return m * out[0] + out[1] + out[2]; // a full cycle
}

} // extern "C"
