// gmres_multi_rule.cpp -- the host rule of multi-right-hand-side GMRES (gmres_multi.hip): the limits, the grid of a pass,
// which preconditioner kinds a batch takes and through which door (precond_rule.h), and the launch counts of a step, a
// close, a restart and start.  No GPU call in this file, so it is testable on a CPU box (and under a host sanitizer).
#include <stdint.h>
#include "../../include/sblas_hip.h"

#pragma clang fp contract(off) // ahead of gmres.h, as everywhere it is included

#include "gmres_multi.h"
#include "precond_rule.h"

extern "C" {

int sblas_gmres_multi_limits(int64_t out[8])
{
    using namespace sblas;
    if (!out) return SBLAS_E_INVALID;
    out[0] = SBLAS_GMRES_MULTI_MAX_RHS, out[1] = TILE, out[2] = KRYLOV_CELL, out[3] = KRYLOV_LANES, out[4] = GMRES_MAX_RESTART;
    out[5] = GMRES_MULTI_FIXED_BLOCKS, out[6] = GMRES_BLOCK_SLOTS, out[7] = GMRES_MULTI_MATRIX_STRIDE;
    return SBLAS_OK;
}

int sblas_gmres_multi_grid(int64_t n, int nrhs, int64_t out[4])
{
    if (!out || n < 0 || !sblas::gmres_multi_width_ok(nrhs)) return SBLAS_E_INVALID;
    out[0] = sblas::krylov_cells(n), out[1] = sblas::tiles(nrhs), out[2] = out[0] * out[1];
    out[3] = nrhs - (int)(out[1] - 1) * sblas::TILE;
    return SBLAS_OK;
}

int sblas_gmres_multi_precond_ok(int precond) { return sblas::precond_multi(precond) ? SBLAS_OK : SBLAS_E_INVALID; }
int sblas_gmres_multi_precond_plan_ok(int precond) { return sblas::precond_multi_applied(precond) ? SBLAS_OK : SBLAS_E_INVALID; }
int sblas_gmres_multi_precond_pair_ok(int precond) { return sblas::precond_multi_pair(precond) ? SBLAS_OK : SBLAS_E_INVALID; }

int64_t sblas_gmres_multi_launches(int restart, int precond, int64_t spmm_launches, int64_t lower_or_cycle_launches, int64_t upper_launches,
                                   int64_t out[4])
{
    if (!sblas::gmres_multi_restart_ok(restart) || !out || spmm_launches < 0) return -1;
    const int64_t apply = sblas::precond_multi_launches(precond, lower_or_cycle_launches, upper_launches); // launches of one block M^-1
    if (apply < 0) return -1;
    // gmres_rule.cpp's counts with the product's launches in the SpMV's place.  step: [M^-1;] SpMM; multi-dot, fold;
    // projection; multi-dot, fold; projection with (w, w); fold and scalar step; normalisation
    out[0] = 8 + spmm_launches + apply;
    out[1] = 3 + apply;         // close: back substitution; combination; [M^-1;] x update
    out[2] = 3 + spmm_launches; // restart: SpMM; residual with (r, r); fold and test; normalisation
    out[3] = 5 + spmm_launches; // start: (b, b), fold; SpMM; residual with (r, r); fold and test; normalisation
    return restart * out[0] + out[1] + out[2];
}

} // extern "C"
