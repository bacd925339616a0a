// precond_rule.h -- the rule of the preconditioner kinds (SBLAS_PRECOND_*), once: which codes are known and what each
// kind asks of a solver.  krylov_rule.cpp and gmres_rule.cpp count launches by it, and the seat a solver plan holds
// (precond.h) decides by it.  No HIP in here: the rule files are testable on a CPU box.  A new kind is added here and
// in precond.h, nowhere else.
#pragma once
#include <stdint.h>
#include "../../include/sblas_hip.h"

namespace sblas {

// applied by launches of its own between the solver's kernels: the two solves, an AMG cycle, a polynomial, FSAI's two
// products.  (Jacobi rides in the solvers' own kernels.)  FSAI's code is 6: 5 stays no kind.
inline bool precond_applied(int kind)
{
    return kind == SBLAS_PRECOND_ILU0 || kind == SBLAS_PRECOND_AMG || kind == SBLAS_PRECOND_CHEBYSHEV || kind == SBLAS_PRECOND_FSAI;
}
inline bool precond_known(int kind) { return kind == SBLAS_PRECOND_NONE || kind == SBLAS_PRECOND_JACOBI || precond_applied(kind); }
// takes the caller's values at start (the inverse diagonal, the factor); the other kinds hold those of their own setup
inline bool precond_takes_values(int kind) { return kind == SBLAS_PRECOND_JACOBI || kind == SBLAS_PRECOND_ILU0; }
// may run with out == in: the two solves go through a temporary; a cycle or a polynomial reads in while it writes out
inline bool precond_in_place(int kind) { return kind == SBLAS_PRECOND_ILU0; }
// serves several right-hand sides at once (krylov_multi.hip): the kinds that ride in the solver's own kernels.  An applied
// kind takes a plan: precond_multi_applied.
inline bool precond_multi(int kind) { return precond_known(kind) && !precond_applied(kind); }
// serves several right-hand sides at once through a plan of its own with a multi-column apply: the AMG
// block cycle.  ILU(0) no longer waits on a row-major sptrsm -- the tiled solve is there -- but it is
// seated as a pair of solve plans, not as one plan: precond_multi_pair.  Chebyshev waits on a block polynomial of its own,
// FSAI on a block apply as two SpMMs.
inline bool precond_multi_applied(int kind) { return kind == SBLAS_PRECOND_AMG; }
// serves several right-hand sides at once through its PAIR of solve plans (sblas_hip_sptrsm_tile.h's create): ILU(0), as
// OUT = L^-1 IN by the tiled solve and OUT = U^-1 OUT in place.  Kept apart from precond_multi_applied, whose answers
// and the refusals of the creates that go by it are pinned.
inline bool precond_multi_pair(int kind) { return kind == SBLAS_PRECOND_ILU0; }
// Launches of one block M^-1 under a multi-right-hand-side plan that takes every door in one create (gmres_multi.hip):
// 0 for a kind that rides in the kernels (and then no launches may be named), the block cycle's for one plan
// (lower_or_cycle, with upper 0), the two tiled solves' for a pair.  -1 for a kind without a multi-column apply, an
// unknown kind or a negative count.
inline int64_t precond_multi_launches(int kind, int64_t lower_or_cycle, int64_t upper)
{
    if (lower_or_cycle < 0 || upper < 0) return -1;
    if (precond_multi(kind)) return lower_or_cycle == 0 && upper == 0 ? 0 : -1;
    if (precond_multi_applied(kind)) return upper == 0 ? lower_or_cycle : -1;
    if (precond_multi_pair(kind)) return lower_or_cycle + upper;
    return -1;
}
// holds two plans, lower and upper; every other applied kind holds one handle in lower's place and no upper
inline bool precond_pair(int kind) { return kind == SBLAS_PRECOND_ILU0; }

// Launches of one M^-1, from [5] of the plans' info (sblas_hip_sptrsv_plan_info of the two solves; with one handle
// sblas_hip_amg_plan_info, one cycle's, sblas_hip_cheby_plan_info, the degree, or sblas_hip_fsai_plan_info, 2).  0 for a kind that is not applied,
// whatever the infos; -1 for an unknown kind, a missing info or a negative [5].
inline int64_t precond_launches(int kind, const int64_t *lower_info, const int64_t *upper_info)
{
    if (!precond_known(kind)) return -1;
    if (!precond_applied(kind)) return 0;
    if (!lower_info || lower_info[5] < 0) return -1;
    if (!precond_pair(kind)) return lower_info[5];
    if (!upper_info || upper_info[5] < 0) return -1;
    return lower_info[5] + upper_info[5];
}

} // namespace sblas
