// fsai_rule.cpp -- the host rule of the FSAI plan (fsai.hip): the pattern of G from A's structure or a
// caller's pattern, and G's values by the scalar loop that is the contract.  Pure functions of host arrays; no GPU call in
// this file, so it is testable on a CPU box (and under a host sanitizer).  The structure check is ILU(0)'s.
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <vector>
#include "../../include/sblas_hip.h"
#include "fsai.h"

#pragma clang fp contract(off) // every product, difference, quotient and square root below is rounded on its own

namespace {

using namespace sblas;

// A[r][c] read from row r of A (ascending): +0.0 where the row stores no such column
double entry(const int32_t *rowptr, const int32_t *colidx, const double *val, int32_t r, int32_t c)
{
    int64_t lo = rowptr[r], hi = rowptr[r + 1];
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (colidx[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo < rowptr[r + 1] && colidx[lo] == c ? val[lo] : 0.0;
}

// One row of G: J (m columns, ascending, the last one the row itself) -> g (m values).  false: the row failed and g is
// the diagonal fallback.  M: room for fsai_triangle(m) doubles, t: for m.
bool row_values(const int32_t *rowptr, const int32_t *colidx, const double *val, const int32_t *J, int m, double *M, double *t, double *g)
{
    for (int p = 0; p < m; ++p)
        for (int q = 0; q <= p; ++q) M[fsai_at(p, q)] = entry(rowptr, colidx, val, J[p], J[q]);
    const double aii = M[fsai_at(m - 1, m - 1)];
    bool ok = true;
    for (int k = 0; k < m && ok; ++k) {
        const double d = M[fsai_at(k, k)];
        if (!fsai_positive(d)) {
            ok = false;
            break;
        }
        const double c = sqrt(d);
        M[fsai_at(k, k)] = c;
        for (int p = k + 1; p < m; ++p) M[fsai_at(p, k)] = M[fsai_at(p, k)] / c;
        for (int p = k + 1; p < m; ++p)
            for (int q = k + 1; q <= p; ++q) {
                const double prod = M[fsai_at(p, k)] * M[fsai_at(q, k)];
                M[fsai_at(p, q)] = M[fsai_at(p, q)] - prod;
            }
    }
    if (!ok) {
        for (int p = 0; p < m - 1; ++p) g[p] = 0.0;
        g[m - 1] = fsai_positive(aii) ? 1.0 / sqrt(aii) : 1.0;
        return false;
    }
    for (int p = 0; p < m; ++p) t[p] = 0.0;
    g[m - 1] = 1.0 / M[fsai_at(m - 1, m - 1)];
    for (int q = m - 1; q >= 1; --q) {
        for (int p = 0; p < q; ++p) {
            const double prod = M[fsai_at(q, p)] * g[q];
            t[p] = t[p] + prod;
        }
        g[q - 1] = (-t[q - 1]) / M[fsai_at(q - 1, q - 1)];
    }
    return true;
}

} // namespace

extern "C" {

int sblas_fsai_limits(int64_t out[8])
{
    if (!out) return SBLAS_E_INVALID;
    out[0] = FSAI_THREADS, out[1] = FSAI_ROW_MAX, out[2] = SPTRSV_G4_MAX, out[3] = SPTRSV_G16_MAX, out[4] = FSAI_TRI_PER_LANE;
    out[5] = FSAI_VEC_PER_LANE, out[6] = FSAI_LDS_BYTES, out[7] = 0;
    return SBLAS_OK;
}

int sblas_fsai_pattern(int64_t n, const int32_t *rowptr, const int32_t *colidx, int64_t nnz_g, const int32_t *rowptr_g, const int32_t *colidx_g,
                       int max_row, int32_t *out_rowptr, int32_t *out_colidx, int64_t *bad_row)
{
    if (bad_row) *bad_row = -1;
    if (n < 0 || n > INT_MAX - 64 || !rowptr || !out_rowptr || !fsai_max_row_ok(max_row)) return SBLAS_E_INVALID;
    if (n > 0 && rowptr[n] > 0 && !colidx) return SBLAS_E_INVALID;
    const bool own = rowptr_g != nullptr;
    if (own ? (nnz_g < 0 || nnz_g > INT_MAX || (nnz_g > 0 && !colidx_g)) : (nnz_g != 0 || colidx_g != nullptr)) return SBLAS_E_INVALID;
    int64_t bad = -1;
    const int rc = sblas_ilu0_check(n, rowptr, colidx, nullptr, &bad);
    if (rc != SBLAS_OK) {
        if (bad_row) *bad_row = bad;
        return rc;
    }
    const auto refuse = [&](int64_t i) {
        if (bad_row) *bad_row = i;
        return SBLAS_E_INVALID;
    };
    const int32_t *srp = own ? rowptr_g : rowptr, *sci = own ? colidx_g : colidx;
    const int64_t snnz = own ? nnz_g : (n > 0 ? rowptr[n] : 0);
    if (own && n > 0 && srp[0] != 0) return refuse(0);
    int64_t fill = 0;
    out_rowptr[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t beg = srp[i], end = srp[i + 1];
        if (beg > end || end > snnz) return refuse(i);
        int64_t m = 0; // the entries with column <= i: a prefix of an ascending row
        bool diagonal = false;
        for (int64_t e = beg; e < end; ++e) {
            const int32_t c = sci[e];
            if (c < 0 || c >= n || (e > beg && c <= sci[e - 1])) return refuse(i);
            if (c <= i) ++m, diagonal = diagonal || c == i;
        }
        if (!diagonal) return refuse(i);
        int64_t keep = m;
        if (max_row > 0 && keep > max_row) keep = max_row; // the diagonal and the max_row - 1 largest columns below it
        if (keep > FSAI_ROW_MAX) return refuse(i);
        if (out_colidx)
            for (int64_t e = beg + m - keep; e < beg + m; ++e) out_colidx[fill + (e - (beg + m - keep))] = sci[e];
        fill += keep;
        out_rowptr[i + 1] = (int32_t)fill;
    }
    if (own && n > 0 && srp[n] != snnz) return refuse(n - 1);
    return SBLAS_OK;
}

int sblas_fsai_ref(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, const int32_t *rowptr_g, const int32_t *colidx_g,
                   double *val_g, int64_t *bad_row)
{
    if (bad_row) *bad_row = -1;
    if (n < 0 || n > INT_MAX - 64 || !rowptr || !rowptr_g) return SBLAS_E_INVALID;
    if (n > 0 && (!colidx || !val || !colidx_g || !val_g)) return SBLAS_E_INVALID;
    int64_t bad = -1;
    const int rc = sblas_ilu0_check(n, rowptr, colidx, nullptr, &bad);
    if (rc != SBLAS_OK) {
        if (bad_row) *bad_row = bad;
        return rc;
    }
    // G's pattern as sblas_fsai_pattern gives it: ascending, at most FSAI_ROW_MAX entries, the last one the diagonal
    if (n > 0 && rowptr_g[0] != 0) return SBLAS_E_INVALID;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t beg = rowptr_g[i], m = (int64_t)rowptr_g[i + 1] - beg;
        if (m < 1 || m > FSAI_ROW_MAX || colidx_g[beg + m - 1] != i) return SBLAS_E_INVALID;
        for (int64_t e = beg; e < beg + m; ++e)
            if (colidx_g[e] < 0 || (e > beg && colidx_g[e] <= colidx_g[e - 1])) return SBLAS_E_INVALID;
    }
    std::vector<double> M((size_t)fsai_triangle(FSAI_ROW_MAX)), t((size_t)FSAI_ROW_MAX);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t beg = rowptr_g[i];
        const int m = (int)(rowptr_g[i + 1] - beg);
        if (!row_values(rowptr, colidx, val, colidx_g + beg, m, M.data(), t.data(), val_g + beg) && bad_row && *bad_row < 0) *bad_row = i;
    }
    return SBLAS_OK;
}

} // extern "C"
