// krylov_multi_rule.cpp -- the host rule of the multi-right-hand-side Krylov solvers (krylov_multi.hip): the limits,
// which preconditioner kinds a batch takes, alone or with a plan (precond_rule.h), the launches of one iteration, the
// grid of a pass, and the scalar step both solvers' folds run (krylov_scalar.h), compiled here for the host.  No GPU call in this file, so it is
// testable on a CPU box (and under a host sanitizer).
#include <stdint.h>
#include "../../include/sblas_hip.h"
#include "krylov.h"
#include "krylov_multi.h"
#include "krylov_scalar.h"
#include "precond_rule.h"

#pragma clang fp contract(off) // as on the device (the step holds nothing to contract)

extern "C" {

int sblas_krylov_multi_limits(int64_t out[8])
{
    if (!out) return SBLAS_E_INVALID;
    out[0] = SBLAS_KRYLOV_MULTI_MAX_RHS, out[1] = sblas::TILE, out[2] = sblas::KRYLOV_CELL, out[3] = sblas::KRYLOV_LANES;
    out[4] = sblas::KRYLOV_PCG_VECTORS, out[5] = sblas::KRYLOV_BICGSTAB_VECTORS, out[6] = sblas::KRYLOV_MAX_DOTS;
    out[7] = sblas::KRYLOV_BLOCK_SLOTS;
    return SBLAS_OK;
}

int sblas_krylov_multi_precond_ok(int precond) { return sblas::precond_multi(precond) ? SBLAS_OK : SBLAS_E_INVALID; }

int64_t sblas_krylov_multi_launches(int method, int precond, int64_t spmm_launches)
{
    if (method != SBLAS_KRYLOV_PCG && method != SBLAS_KRYLOV_BICGSTAB) return -1;
    if (!sblas::precond_multi(precond) || spmm_launches < 0) return -1;
    // PCG: SpMM; (p, q): stage 1, fold; x / r update; fold; p update
    if (method == SBLAS_KRYLOV_PCG) return spmm_launches + 5;
    // p update; SpMM; (r^, v): stage 1, fold; s update; SpMM; (t, s), (t, t) and (s, s): stage 1, fold; x / r update; fold
    return 2 * spmm_launches + 8;
}

int sblas_krylov_multi_precond_plan_ok(int precond) { return sblas::precond_multi_applied(precond) ? SBLAS_OK : SBLAS_E_INVALID; }

int64_t sblas_krylov_multi_launches_ex(int method, int precond, int64_t spmm_launches, int64_t precond_launches)
{
    if (precond_launches < 0) return -1;
    if (sblas::precond_multi(precond)) return precond_launches == 0 ? sblas_krylov_multi_launches(method, precond, spmm_launches) : -1;
    if (!sblas::precond_multi_applied(precond)) return -1;
    const int64_t plain = sblas_krylov_multi_launches(method, SBLAS_PRECOND_NONE, spmm_launches);
    if (plain < 0) return -1;
    // PCG: after the residual's fold the block apply, the dots (r, z): stage 1, and the fold that takes beta (krylov.hip's
    // pcg_iteration); BiCGStab: the block apply on P and on S
    return method == SBLAS_KRYLOV_PCG ? plain + precond_launches + 2 : plain + 2 * precond_launches;
}

int sblas_krylov_multi_precond_pair_ok(int precond) { return sblas::precond_multi_pair(precond) ? SBLAS_OK : SBLAS_E_INVALID; }

int64_t sblas_krylov_multi_launches_pair(int method, int precond, int64_t spmm_launches, int64_t lower_launches, int64_t upper_launches)
{
    if (!sblas::precond_multi_pair(precond) || lower_launches < 0 || upper_launches < 0) return -1;
    const int64_t plain = sblas_krylov_multi_launches(method, SBLAS_PRECOND_NONE, spmm_launches);
    if (plain < 0) return -1;
    // the count with a block cycle seated (above), the two solves' launches in the cycle's place
    const int64_t apply = lower_launches + upper_launches;
    return method == SBLAS_KRYLOV_PCG ? plain + apply + 2 : plain + 2 * apply;
}

int sblas_krylov_multi_grid(int64_t n, int nrhs, int64_t out[4])
{
    if (!out || n < 0 || !sblas::krylov_multi_width_ok(nrhs)) return SBLAS_E_INVALID;
    out[0] = sblas::krylov_cells(n), out[1] = sblas::tiles(nrhs), out[2] = out[0] * out[1];
    out[3] = nrhs - (int)(out[1] - 1) * sblas::TILE;
    return SBLAS_OK;
}

int sblas_krylov_scalar_step_ref(int op, int nd, int flag, const double *d, double *block, double rtol, double atol, int64_t max_iter)
{
    if (op < SBLAS_KRYLOV_STEP_START_B || op > SBLAS_KRYLOV_STEP_BICG_RES || nd < 1 || nd > sblas::KRYLOV_MAX_DOTS || !d || !block)
        return SBLAS_E_INVALID;
    if (op == SBLAS_KRYLOV_STEP_BICG_OMEGA && nd < 3) return SBLAS_E_INVALID; // reads (t, s), (t, t) and (s, s)
    if (op == SBLAS_KRYLOV_STEP_BICG_RES && nd < 2) return SBLAS_E_INVALID;   // reads (r, r) and (r^, r)
    sblas::krylov_scalar_step(op, nd, flag, d, block, rtol, atol, (long long)max_iter);
    return SBLAS_OK;
}

} // extern "C"
