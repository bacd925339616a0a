// ilu0_plan.cpp -- the host rule of the ILU(0) plan (sblas_hip_ilu0_plan_create, ilu0.hip): the structure check and the
// limits.  Pure functions of host arrays; no GPU call in this file, so it is testable on a CPU box.  The levels, the
// packing into lane units and the launches are the triangular solves' (sblas_sptrsv_levels with LOWER and NON_UNIT,
// level_plan.h): row i of the factor needs the finished rows k < i it stores an entry for, which is exactly what row i
// of a lower solve needs.
#include <limits.h>
#include <stdint.h>
#include "../../include/sblas_hip.h"
#include "ilu0.h"

extern "C" {

int sblas_hip_ilu0_limits(int64_t out[6])
{
    if (!out) return SBLAS_E_INVALID;
    out[0] = sblas::ILU0_CHAIN_ROWS, out[1] = sblas::ILU0_CHAIN_THREADS, out[2] = sblas::SPTRSV_G4_MAX, out[3] = sblas::SPTRSV_G16_MAX;
    out[4] = sblas::ILU0_LDS_MAX, out[5] = sblas::ILU0_WIDE_THREADS;
    return SBLAS_OK;
}

int sblas_ilu0_check(int64_t n, const int32_t *rowptr, const int32_t *colidx, int32_t *diag_pos_out, int64_t *bad_row)
{
    if (bad_row) *bad_row = -1;
    if (n < 0 || n > INT_MAX || !rowptr) return SBLAS_E_INVALID;
    const auto refuse = [&](int64_t row) {
        if (bad_row) *bad_row = row;
        return SBLAS_E_INVALID;
    };
    // the row pointers first: nothing indexes colidx before they are known to be sound
    if (rowptr[0] != 0) return refuse(0);
    for (int64_t i = 0; i < n; ++i)
        if (rowptr[i + 1] < rowptr[i]) return refuse(i);
    if (n > 0 && rowptr[n] > 0 && !colidx) return SBLAS_E_INVALID;
    // then every column's range, in every row
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e)
            if (colidx[e] < 0 || colidx[e] >= n) return refuse(i);
    // then row by row: strictly ascending columns (sorted, nothing doubled) and a stored diagonal
    for (int64_t i = 0; i < n; ++i) {
        int64_t dpos = -1;
        for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
            if (e > rowptr[i] && colidx[e] <= colidx[e - 1]) return refuse(i);
            if (colidx[e] == i) dpos = e;
        }
        if (dpos < 0) return refuse(i);
        if (diag_pos_out) diag_pos_out[i] = (int32_t)dpos;
    }
    return SBLAS_OK;
}

} // extern "C"
