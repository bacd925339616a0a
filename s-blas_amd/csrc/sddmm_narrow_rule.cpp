// sddmm_narrow_rule.cpp -- the host side of the narrow SDDMM (sddmm_narrow.hip): the sizes the kernel is built on and the
// contract of include/sblas_hip_sddmm_narrow.h as a scalar loop, on the definitions the kernel uses (sddmm_narrow.h).  No
// GPU call in this file, so it is testable on a CPU box (tools/sddmm_narrow_rule_check.cpp builds it alone under a host
// sanitizer).
#include <limits.h>
#include <stdint.h>
#include "../../include/sblas_hip.h"
#include "sddmm_narrow.h"

extern "C" {

int sblas_sddmm_narrow_limits(int64_t out[4])
{
    if (!out) return SBLAS_E_INVALID;
    out[0] = sblas::SDDMM_NARROW_MAX_K, out[1] = sblas::SDDMM_NARROW_CHUNK;
    out[2] = sblas::SDDMM_NARROW_THREADS, out[3] = sblas::SDDMM_NARROW_EPL;
    return SBLAS_OK;
}

int sblas_sddmm_narrow_ref(int, void *, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                           const double *X, int64_t ldx, const double *Y, int64_t ldy, int k, double alpha, double beta,
                           int part, double *out)
{
    if (rows < 0 || cols < 0 || nnz < 0 || rows > INT_MAX - 64 || cols > INT_MAX || nnz > INT_MAX) return SBLAS_E_INVALID;
    if (k < 1 || k > sblas::SDDMM_NARROW_MAX_K || ldx < k || ldy < k || !sblas::sddmm_narrow_part_ok(part)) return SBLAS_E_INVALID;
    if (!rowptr || (nnz > 0 && (!colidx || !out || !X || !Y))) return SBLAS_E_INVALID;
    if (nnz > 0 && (rows == 0 || cols == 0)) return SBLAS_E_INVALID; // entries without a place
    if (rowptr[0] != 0 || rowptr[rows] != nnz) return SBLAS_E_INVALID;
    for (int64_t i = 0; i < rows; ++i)
        if (rowptr[i + 1] < rowptr[i]) return SBLAS_E_INVALID;
    for (int64_t e = 0; e < nnz; ++e)
        if (colidx[e] < 0 || colidx[e] >= cols) return SBLAS_E_INVALID;
    const int kp = sblas::sddmm_narrow_padded(k);
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t e = rowptr[r]; e < rowptr[r + 1]; ++e) {
            const int c = colidx[e];
            const bool inside = sblas::sddmm_narrow_in_part(part, (int)r, c);
            double x[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, y[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (inside) // the rows of an entry outside the part are never read
                for (int j = 0; j < k; ++j) x[j] = X[r * ldx + j], y[j] = Y[(int64_t)c * ldy + j];
            const double s = inside ? sblas::sddmm_narrow_dot(x, y, kp) : 0.0;
            out[e] = sblas::sddmm_narrow_out(inside, s, alpha, beta, beta == 0.0 ? 0.0 : out[e]);
        }
    return SBLAS_OK;
}

} // extern "C"
