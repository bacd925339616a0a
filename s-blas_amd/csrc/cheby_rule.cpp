// cheby_rule.cpp -- the host rule of the Chebyshev plan (cheby.hip): the start vector, the Lanczos
// recurrence of the eigenvalue estimate, the Ritz value, the row bound, the coefficient table and the polynomial itself
// restated in plain C++.  Pure functions of host arrays; no GPU call in this file, so it is testable on a CPU box (and
// under a host sanitizer).  The scalar routine is cheby.h's, the text the device compiles; the row sum is amg.h's and the
// dot sblas_krylov_dot_ref.
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <vector>
#include "../../include/sblas_hip.h"
#include "amg.h"
#include "cheby.h"
#include "color.h"

#pragma clang fp contract(off) // every product, sum, quotient and difference below is rounded on its own

namespace {

using namespace sblas;

// the structure contract (rows strictly ascending, a stored diagonal) and the diagonal's places
int checked(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, std::vector<int32_t> &dpos, int64_t *bad_row)
{
    if (bad_row) *bad_row = -1;
    if (n < 0 || n > INT_MAX || !rowptr) return SBLAS_E_INVALID;
    if (n > 0 && rowptr[n] > 0 && (!colidx || !val)) return SBLAS_E_INVALID;
    dpos.resize((size_t)n);
    return sblas_ilu0_check(n, rowptr, colidx, dpos.data(), bad_row);
}

// dinv_i = 1 / a_ii; the least row whose diagonal is not finite and > 0 is reported, as the device flags it
void inverse_diagonal(int64_t n, const std::vector<int32_t> &dpos, const double *val, std::vector<double> &dinv, int64_t *bad_row)
{
    dinv.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const double d = val[dpos[(size_t)i]];
        dinv[(size_t)i] = 1.0 / d;
        if (!cheby_positive(d) && bad_row && *bad_row < 0) *bad_row = i;
    }
}

void start_vector(int64_t n, uint32_t seed, uint32_t level, double *b0)
{
    const uint32_t salt = color_salt(seed + level);
    for (int64_t i = 0; i < n; ++i) b0[i] = cheby_start_value(color_priority((uint32_t)i, salt));
}

} // namespace

extern "C" {

int sblas_cheby_limits(int64_t out[8])
{
    if (!out) return SBLAS_E_INVALID;
    out[0] = CHEBY_THREADS, out[1] = CHEBY_MAX_DEGREE, out[2] = CHEBY_MAX_STEPS, out[3] = CHEBY_DEFAULT_DEGREE, out[4] = CHEBY_DEFAULT_STEPS;
    out[5] = CHEBY_BISECTIONS, out[6] = CHEBY_BLOCK_SLOTS, out[7] = 0;
    return SBLAS_OK;
}

int sblas_cheby_start_ref(int64_t n, uint32_t seed, uint32_t level, double *b0)
{
    if (n < 0 || n > INT_MAX || (n > 0 && !b0)) return SBLAS_E_INVALID;
    start_vector(n, seed, level, b0);
    return SBLAS_OK;
}

int sblas_cheby_lanczos_ref(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, uint32_t seed, uint32_t level,
                            int steps, double *alpha, double *beta, int64_t *m, int64_t *bad_row)
{
    if (m) *m = 0;
    if (!cheby_steps_ok(steps) || !alpha || !beta || !m) {
        if (bad_row) *bad_row = -1;
        return SBLAS_E_INVALID;
    }
    std::vector<int32_t> dpos;
    const int rc = checked(n, rowptr, colidx, val, dpos, bad_row);
    if (rc != SBLAS_OK) return rc;
    std::vector<double> dinv, r((size_t)n), z((size_t)n), p((size_t)n), q((size_t)n);
    inverse_diagonal(n, dpos, val, dinv, bad_row);
    start_vector(n, seed, level, r.data());
    for (int64_t i = 0; i < n; ++i) z[(size_t)i] = dinv[(size_t)i] * r[(size_t)i], p[(size_t)i] = z[(size_t)i];
    double rho = sblas_krylov_dot_ref(n, r.data(), z.data());
    for (int j = 0; j < steps; ++j) {
        for (int64_t i = 0; i < n; ++i) q[(size_t)i] = amg_row_sum(colidx, val, rowptr[i], rowptr[i + 1], p.data());
        const double pq = sblas_krylov_dot_ref(n, p.data(), q.data());
        if (!cheby_positive(pq)) break;
        const double a = rho / pq;
        if (!cheby_positive(a)) break;
        alpha[j] = a, *m = j + 1;
        if (j == steps - 1) break;
        for (int64_t i = 0; i < n; ++i) {
            const double step = a * q[(size_t)i];
            r[(size_t)i] = r[(size_t)i] - step;
            z[(size_t)i] = dinv[(size_t)i] * r[(size_t)i];
        }
        const double rho_new = sblas_krylov_dot_ref(n, r.data(), z.data());
        const double b = rho_new / rho;
        if (!cheby_positive(b)) break;
        beta[j] = b, rho = rho_new;
        for (int64_t i = 0; i < n; ++i) {
            const double carried = b * p[(size_t)i];
            p[(size_t)i] = z[(size_t)i] + carried;
        }
    }
    return SBLAS_OK;
}

int sblas_cheby_ritz_ref(int m, const double *alpha, const double *beta, double *t, double *e2, double *ritz)
{
    if (m < 1 || m > CHEBY_MAX_STEPS || !alpha || (m > 1 && !beta) || !ritz) return SBLAS_E_INVALID;
    double tt[CHEBY_MAX_STEPS], ee[CHEBY_MAX_STEPS];
    cheby_tridiagonal(m, alpha, beta, tt, ee);
    *ritz = cheby_ritz(m, tt, ee);
    for (int j = 0; j < m; ++j) {
        if (t) t[j] = tt[j];
        if (e2 && j < m - 1) e2[j] = ee[j];
    }
    return SBLAS_OK;
}

int sblas_cheby_rowbound_ref(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, double *g, int64_t *bad_row)
{
    if (!g) {
        if (bad_row) *bad_row = -1;
        return SBLAS_E_INVALID;
    }
    *g = 0.0;
    std::vector<int32_t> dpos;
    const int rc = checked(n, rowptr, colidx, val, dpos, bad_row);
    if (rc != SBLAS_OK) return rc;
    double most = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        double s = 0.0;
        for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) s = s + fabs(val[e]);
        const double d = val[dpos[(size_t)i]], bound = s / d;
        if (bound > most) most = bound; // a NaN is never the maximum
        if (!cheby_positive(d) && bad_row && *bad_row < 0) *bad_row = i;
    }
    *g = most;
    return SBLAS_OK;
}

double sblas_cheby_lambda_ref(int64_t m, double ritz, double g, double boost) { return cheby_lambda_max(m, ritz, g, boost); }

int sblas_cheby_coef_ref(double lambda_max, double ratio, int degree, double *table, double *lambda_min)
{
    if (!cheby_degree_ok(degree) || !cheby_ratio_ok(ratio) || lambda_max != lambda_max || !table) return SBLAS_E_INVALID;
    const double low = lambda_max / ratio;
    if (lambda_min) *lambda_min = low;
    cheby_coefficients(lambda_max, low, degree, table);
    return SBLAS_OK;
}

int sblas_cheby_apply_ref(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, const double *table, int degree,
                          const double *b, const double *x, double *y, int64_t *bad_row)
{
    if (!cheby_degree_ok(degree) || !table) {
        if (bad_row) *bad_row = -1;
        return SBLAS_E_INVALID;
    }
    std::vector<int32_t> dpos;
    const int rc = checked(n, rowptr, colidx, val, dpos, bad_row);
    if (rc != SBLAS_OK) return rc;
    if (n > 0 && (!b || !y || y == b || y == x)) return SBLAS_E_INVALID;
    std::vector<double> dinv, d((size_t)n), cur((size_t)n), next((size_t)n);
    inverse_diagonal(n, dpos, val, dinv, bad_row);
    for (int64_t i = 0; i < n; ++i) { // step 0: the old d is not read
        if (x) {
            const double res = b[i] - amg_row_sum(colidx, val, rowptr[i], rowptr[i + 1], x);
            const double t = dinv[(size_t)i] * res;
            d[(size_t)i] = table[1] * t;
            cur[(size_t)i] = x[i] + d[(size_t)i];
        } else {
            const double t = dinv[(size_t)i] * b[i];
            d[(size_t)i] = table[1] * t;
            cur[(size_t)i] = d[(size_t)i];
        }
    }
    for (int k = 1; k < degree; ++k) {
        for (int64_t i = 0; i < n; ++i) {
            const double res = b[i] - amg_row_sum(colidx, val, rowptr[i], rowptr[i + 1], cur.data());
            const double t = dinv[(size_t)i] * res;
            const double kept = table[2 * k] * d[(size_t)i], added = table[2 * k + 1] * t;
            d[(size_t)i] = kept + added;
            next[(size_t)i] = cur[(size_t)i] + d[(size_t)i];
        }
        cur.swap(next);
    }
    for (int64_t i = 0; i < n; ++i) y[i] = cur[(size_t)i];
    return SBLAS_OK;
}

} // extern "C"
