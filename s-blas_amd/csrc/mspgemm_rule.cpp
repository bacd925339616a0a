// mspgemm_rule.cpp -- the host side of the masked SpGEMM plan (sblas_hip_mspgemm_plan_create, mspgemm.hip): the limits its
// kernels are built on and the contract of include/sblas_hip_mspgemm.h as a scalar loop.  No GPU call in this file, so it
// is testable on a CPU box (tools/mspgemm_rule_check.cpp builds it alone under a host sanitizer).
#include <limits.h>
#include <stdint.h>
#include "../../include/sblas_hip.h"
#include "mspgemm.h"

// x * y and p1 + p2 are separate roundings
#pragma clang fp contract(off)

namespace {

// rowptr starts at 0 and never steps down; every column of its nnz entries is inside [0, cols)
bool structure_ok(int64_t rows, int64_t cols, const int32_t *rowptr, const int32_t *colidx)
{
    if (!rowptr || rowptr[0] != 0) return false;
    for (int64_t i = 0; i < rows; ++i)
        if (rowptr[i + 1] < rowptr[i]) return false;
    const int64_t nnz = rowptr[rows];
    if (nnz > 0 && !colidx) return false;
    for (int64_t e = 0; e < nnz; ++e)
        if (colidx[e] < 0 || (int64_t)colidx[e] >= cols) return false;
    return true;
}

} // namespace

extern "C" {

int sblas_mspgemm_limits(int64_t out[4])
{
    if (!out) return SBLAS_E_INVALID;
    out[0] = sblas::MSPGEMM_LDS_ROW, out[1] = sblas::MSPGEMM_THREADS, out[2] = 0, out[3] = 0;
    return SBLAS_OK;
}

int sblas_mspgemm_ref(int64_t m, int64_t n, int64_t k, const int32_t *rowptr_m, const int32_t *colidx_m, const int32_t *rowptr_x,
                      const int32_t *colidx_x, const double *val_x, const int32_t *rowptr_y, const int32_t *colidx_y, const double *val_y,
                      double *out)
{
    if (m < 0 || n < 0 || k < 0 || m > INT_MAX || n > INT_MAX || k > INT_MAX) return SBLAS_E_INVALID;
    if (!structure_ok(m, n, rowptr_m, colidx_m) || !structure_ok(m, k, rowptr_x, colidx_x) || !structure_ok(n, k, rowptr_y, colidx_y))
        return SBLAS_E_INVALID;
    if ((rowptr_m[m] > 0 && !out) || (rowptr_x[m] > 0 && !val_x) || (rowptr_y[n] > 0 && !val_y)) return SBLAS_E_INVALID;
    for (int64_t i = 0; i < m; ++i) {
        for (int64_t t = rowptr_m[i]; t < rowptr_m[i + 1]; ++t) {
            const int64_t j = colidx_m[t];
            double acc = 0.0; // no pair: +0.0
            bool first = true;
            for (int64_t e = rowptr_x[i]; e < rowptr_x[i + 1]; ++e) {
                for (int64_t g = rowptr_y[j]; g < rowptr_y[j + 1]; ++g) {
                    if (colidx_x[e] != colidx_y[g]) continue;
                    const double p = val_x[e] * val_y[g];
                    acc = first ? p : acc + p; // a single product is copied
                    first = false;
                }
            }
            out[t] = acc;
        }
    }
    return SBLAS_OK;
}

} // extern "C"
