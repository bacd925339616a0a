// precond.h -- the seat a solver plan (krylov.hip, gmres.hip; through multi_plan.h's base krylov_multi.hip and
// gmres_multi.hip) holds for its preconditioner, and the SpMV of such a plan.
// The seat answers the five questions a solver asks -- may this be seated (bind), whose values does it take at start
// (take), what does it cost (info), apply it, and the predicates of the iteration code -- so that a solver names no kind
// but NONE and JACOBI, which live in its own kernels.  A new kind is added here and in precond_rule.h.
// Internal to each translation unit, as capi_util.h.
#pragma once
#include "capi_util.h"
#include "precond_rule.h"

namespace {

struct PrecondSeat {
    int kind = SBLAS_PRECOND_NONE;
    // the caller's plans: ILU(0)'s two solves; an AMG, a Chebyshev or an FSAI plan's handle sits in lower, with upper NULL
    const void *lower = nullptr, *upper = nullptr;
    const int32_t *rowptr = nullptr, *colidx = nullptr; // the structure the solves read
    const double *values = nullptr; // start's lu_or_dinv: the factor or the inverse diagonal; nullptr where the kind holds its own

    bool none() const { return kind == SBLAS_PRECOND_NONE; }
    bool jacobi() const { return kind == SBLAS_PRECOND_JACOBI; }
    bool applied() const { return sblas::precond_applied(kind); }
    bool in_place() const { return sblas::precond_in_place(kind); }

    // create: the plans must be the ones the kind asks for, made on `device` for this very structure
    int bind(int precond, const void *lower_plan, const void *upper_plan, int device, int64_t n, int64_t nnz, const int32_t *rp, const int32_t *ci)
    {
        if (!sblas::precond_known(precond)) return SBLAS_E_INVALID;
        if (sblas::precond_pair(precond)) {
            if (!lower_plan || !upper_plan) return SBLAS_E_INVALID;
            const void *plans[2] = {lower_plan, upper_plan};
            const int fill[2] = {SBLAS_FILL_LOWER, SBLAS_FILL_UPPER}, diag[2] = {SBLAS_DIAG_UNIT, SBLAS_DIAG_NON_UNIT};
            for (int k = 0; k < 2; ++k) {
                int64_t info[12];
                if (sblas_hip_sptrsv_plan_info(plans[k], info) != SBLAS_OK) return SBLAS_E_INVALID;
                if (info[0] != n || info[1] != nnz || info[2] != fill[k] || info[3] != diag[k]) return SBLAS_E_INVALID;
                if (sblas_hip_sptrsv_plan_speaks_for(plans[k], device, rp, ci) != SBLAS_OK) return SBLAS_E_INVALID;
            }
        } else if (sblas::precond_applied(precond)) {
            if (!lower_plan || upper_plan) return SBLAS_E_INVALID;
            const int rc = precond == SBLAS_PRECOND_AMG    ? sblas_hip_amg_plan_speaks_for(lower_plan, device, n, nnz, rp, ci)
                           : precond == SBLAS_PRECOND_FSAI ? sblas_hip_fsai_plan_speaks_for(lower_plan, device, n, nnz, rp, ci)
                                                           : sblas_hip_cheby_plan_speaks_for(lower_plan, device, n, nnz, rp, ci);
            if (rc != SBLAS_OK) return SBLAS_E_INVALID;
        } else if (lower_plan || upper_plan) {
            return SBLAS_E_INVALID;
        }
        kind = precond, lower = lower_plan, upper = upper_plan, rowptr = rp, colidx = ci;
        return SBLAS_OK;
    }

    // start: false when the kind needs the caller's values and there are none
    bool take(const double *lu_or_dinv)
    {
        const bool takes = sblas::precond_takes_values(kind);
        if (takes && !lu_or_dinv) return false;
        values = takes ? lu_or_dinv : nullptr;
        return true;
    }

    // plan_info: the out[12] of the seated plans' info, zeros where there is none
    void info(int64_t lower_info[12], int64_t upper_info[12]) const
    {
        for (int k = 0; k < 12; ++k) lower_info[k] = upper_info[k] = 0;
        if (kind == SBLAS_PRECOND_ILU0) sblas_hip_sptrsv_plan_info(lower, lower_info), sblas_hip_sptrsv_plan_info(upper, upper_info);
        else if (kind == SBLAS_PRECOND_AMG) sblas_hip_amg_plan_info(lower, lower_info);
        else if (kind == SBLAS_PRECOND_CHEBYSHEV) sblas_hip_cheby_plan_info(lower, lower_info);
        else if (kind == SBLAS_PRECOND_FSAI) sblas_hip_fsai_plan_info(lower, lower_info);
    }

    // out = M^-1 in, for an applied kind.  ILU(0): out = U^-1 (L^-1 in) through tmp with the factor start was given; out
    // may be in.  AMG: one cycle, Chebyshev: the polynomial, FSAI: z = G^T (G r), each with the values of its own setup; tmp stays unused
    // and out must not overlap in (in_place() says which).
    int apply(hipStream_t s, const double *in, double *tmp, double *out) const
    {
        if (kind == SBLAS_PRECOND_AMG) return sblas_hip_amg_plan_apply(lower, s, in, out);
        if (kind == SBLAS_PRECOND_CHEBYSHEV) return sblas_hip_cheby_plan_apply(lower, s, in, out);
        if (kind == SBLAS_PRECOND_FSAI) return sblas_hip_fsai_plan_apply(lower, s, in, out);
        const int rc = sblas_hip_sptrsv_f64_i32_planned(lower, s, rowptr, colidx, values, 1.0, in, tmp);
        if (rc != SBLAS_OK) return rc;
        return sblas_hip_sptrsv_f64_i32_planned(upper, s, rowptr, colidx, values, 1.0, tmp, out);
    }

    // OUT = M^-1 IN on n x s row-major blocks, for a kind with a multi-column apply (precond_multi_applied): the AMG block
    // cycle, or with a pair of solve plans (precond_multi_pair): ILU(0), OUT = L^-1 IN by the tiled solve and then
    // OUT = U^-1 OUT in place, with the factor start was given.  Column j has apply()'s bits on column j either way.  OUT
    // must not overlap IN, except that a kind with in_place() takes OUT == IN at one leading dimension: both tiled solves
    // then run in place.
    int apply_multi(hipStream_t s, int nrhs, const double *in, int64_t ldin, double *out, int64_t ldout) const
    {
        if (sblas::precond_multi_pair(kind)) {
            const int rc = sblas_hip_sptrsm_tiled_f64_i32_planned(lower, s, rowptr, colidx, values, nrhs, 1.0, in, ldin, out, ldout);
            if (rc != SBLAS_OK) return rc;
            return sblas_hip_sptrsm_tiled_f64_i32_planned(upper, s, rowptr, colidx, values, nrhs, 1.0, out, ldout, out, ldout);
        }
        if (kind != SBLAS_PRECOND_AMG) return SBLAS_E_INVALID;
        return sblas_hip_amg_plan_apply_multi(lower, s, nrhs, in, ldin, out, ldout);
    }
};

// y = A x of a solver plan: through its SpMV plan where it was given one
template <typename Plan> int plan_spmv(const Plan *p, hipStream_t s, const double *x, double *y)
{
    if (p->spmv)
        return sblas_hip_spmv_csr_f64_i32_planned(p->spmv, -1, s, p->n, p->n, p->nnz, p->rowptr, p->colidx, p->val, x, 1.0, 0.0, y);
    return sblas_hip_spmv_csr_f64_i32(-1, s, p->n, p->n, p->nnz, p->rowptr, p->colidx, p->val, x, 1.0, 0.0, y);
}

} // namespace
