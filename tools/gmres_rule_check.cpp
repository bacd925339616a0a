// gmres_rule_check.cpp -- a stand-alone program over GMRES's host rule (s-blas_amd/csrc/gmres_rule.cpp; no GPU, no HIP
// runtime), made to be built with a host sanitizer:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/gmres_rule_check.cpp s-blas_amd/csrc/gmres_rule.cpp -o /tmp/gmres_rule_check && /tmp/gmres_rule_check
// It runs whole cycles of scalar steps for every restart length m from 1 to 64 out of arrays of exactly the sizes the
// contract names (so a read or write past either end is the sanitizer's to find), compares each step with a second
// restatement of the written order, takes the back substitution at k = 0, 1 and m, and puts a zero and a NaN into d.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../include/sblas_hip.h"

#pragma clang fp contract(off)

static uint64_t state = 88172645463325252ull;
static double rnd()
{
    state ^= state << 13, state ^= state >> 7, state ^= state << 17;
    return (double)(int64_t)(state >> 11) / 9007199254740992.0 - 0.5;
}

static bool same(double a, double b) { return memcmp(&a, &b, 8) == 0 || (isnan(a) && isnan(b)); }

// the written order once more, on vectors that grow as the contract says they do
static int restated(int j, std::vector<double> &h, double eta, std::vector<double> &c, std::vector<double> &s, std::vector<double> &g,
                    std::vector<double> &rcol, double tol, int64_t max_iter, int64_t &iter, double &rnorm)
{
    for (int i = 0; i < j; ++i) {
        const double a = c[(size_t)i] * h[(size_t)i], b = s[(size_t)i] * h[(size_t)i + 1], t = a + b;
        const double p = (-s[(size_t)i]) * h[(size_t)i], q = c[(size_t)i] * h[(size_t)i + 1];
        h[(size_t)i + 1] = p + q;
        h[(size_t)i] = t;
    }
    const double hh = h[(size_t)j] * h[(size_t)j], ee = eta * eta, d = sqrt(hh + ee);
    if (d == 0.0 || !isfinite(d)) return SBLAS_KRYLOV_BREAKDOWN;
    c.push_back(h[(size_t)j] / d), s.push_back(eta / d);
    rcol.assign(h.begin(), h.begin() + j);
    rcol.push_back(d);
    g.push_back((-s[(size_t)j]) * g[(size_t)j]);
    g[(size_t)j] = c[(size_t)j] * g[(size_t)j];
    rnorm = fabs(g[(size_t)j + 1]);
    ++iter;
    if (rnorm <= tol) return SBLAS_KRYLOV_CONVERGED;
    return iter >= max_iter ? SBLAS_KRYLOV_LIMIT : SBLAS_KRYLOV_RUNNING;
}

int main()
{
    int bad = 0;
    int64_t lim[8];
    if (sblas_gmres_limits(lim) != SBLAS_OK || sblas_gmres_limits(nullptr) != SBLAS_E_INVALID) return 1;
    const int M = (int)lim[0];
    bad += M != SBLAS_GMRES_MAX_RESTART || lim[2] != M + 1 || lim[1] < 1 || lim[1] > M;
    for (int m = 1; m <= M; ++m) {
        // the arrays of one cycle, exactly as long as a cycle of m steps may touch
        std::vector<double> c((size_t)m), s((size_t)m), g((size_t)m + 1), R((size_t)m * (size_t)m, 0.0);
        std::vector<double> rc, rs, rg(1);
        g[0] = rg[0] = 1.0 + rnd();
        int64_t iter = 0, riter = 0;
        for (int j = 0; j < m; ++j) { // j at both ends and everything between
            std::vector<double> h((size_t)j + 1), rh, rcol((size_t)j + 1), rrcol;
            for (double &v : h) v = ldexp(rnd(), (int)(state % 40) - 20);
            rh = h;
            const double eta = fabs(rnd()) + 0.125;
            double rnorm = -1.0, rrnorm = -1.0;
            int64_t which = 0;
            const int64_t max_iter = j == m - 1 ? m : 1000; // the last step meets the limit
            const int st = sblas_gmres_step_ref(j, h.data(), eta, c.data(), s.data(), g.data(), rcol.data(), 0.0, max_iter, &iter, &rnorm, &which);
            const int want = restated(j, rh, eta, rc, rs, rg, rrcol, 0.0, max_iter, riter, rrnorm);
            bool ok = st == want && st == (j == m - 1 ? SBLAS_KRYLOV_LIMIT : SBLAS_KRYLOV_RUNNING) && iter == riter && same(rnorm, rrnorm) && which == 0;
            for (int i = 0; i <= j && ok; ++i) ok = same(h[(size_t)i], rh[(size_t)i]) && same(rcol[(size_t)i], rrcol[(size_t)i]) && same(c[(size_t)i], rc[(size_t)i]) && same(s[(size_t)i], rs[(size_t)i]);
            for (int i = 0; i <= j + 1 && ok; ++i) ok = same(g[(size_t)i], rg[(size_t)i]);
            if (!ok) {
                printf("m = %d, j = %d: the step differs from its restatement (status %d, want %d)\n", m, j, st, want);
                ++bad;
            }
            for (int i = 0; i <= j; ++i) R[(size_t)j * (size_t)m + (size_t)i] = rcol[(size_t)i];
        }
        // the back substitution at k = 0, 1 and m, with y of exactly k entries and R of leading dimension m
        const int ks[3] = {0, 1, m};
        for (int k : ks) {
            std::vector<double> y((size_t)k), ry((size_t)k);
            if (sblas_gmres_solve_ref(k, k ? R.data() : nullptr, m, k ? g.data() : nullptr, k ? y.data() : nullptr) != SBLAS_OK) ++bad;
            for (int i = k - 1; i >= 0; --i) {
                double t = g[(size_t)i];
                for (int l = i + 1; l < k; ++l) {
                    const double p = R[(size_t)l * (size_t)m + (size_t)i] * ry[(size_t)l];
                    t = t - p;
                }
                ry[(size_t)i] = t / R[(size_t)i * (size_t)m + (size_t)i];
            }
            for (int i = 0; i < k; ++i)
                if (!same(y[(size_t)i], ry[(size_t)i])) {
                    printf("m = %d, k = %d: y[%d] = %a, restated %a\n", m, k, i, y[(size_t)i], ry[(size_t)i]);
                    ++bad;
                    break;
                }
        }
        // a zero and a NaN in d at the last step of this length: a breakdown that changes nothing but h
        const int j = m - 1;
        const double etas[2] = {0.0, NAN};
        for (double eta : etas) {
            std::vector<double> h((size_t)j + 1, 0.0), c2(c.begin(), c.begin() + j), s2(s.begin(), s.begin() + j), g2(g.begin(), g.begin() + j + 1);
            std::vector<double> rcol((size_t)j + 1, -7.0);
            c2.push_back(-7.0), s2.push_back(-7.0), g2.push_back(-7.0);
            int64_t it = j, which = 0;
            double rnorm = -7.0;
            const double gj = g2[(size_t)j];
            const int st = sblas_gmres_step_ref(j, h.data(), eta, c2.data(), s2.data(), g2.data(), rcol.data(), INFINITY, 1000, &it, &rnorm, &which);
            if (st != SBLAS_KRYLOV_BREAKDOWN || which != SBLAS_GMRES_DENOM_GIVENS || it != j || rnorm != -7.0 || c2[(size_t)j] != -7.0 ||
                s2[(size_t)j] != -7.0 || g2[(size_t)j + 1] != -7.0 || !same(g2[(size_t)j], gj) || rcol[(size_t)j] != -7.0) {
                printf("m = %d: d from eta = %g did not break down cleanly (status %d)\n", m, eta, st);
                ++bad;
            }
        }
    }
    // the lucky breakdown: eta == 0 with d != 0 converges at tolerance 0
    {
        double h[1] = {3.0}, c[1], s[1], g[2] = {2.0, -7.0}, rcol[1], rnorm = -1.0;
        int64_t it = 0, which = 0;
        const int st = sblas_gmres_step_ref(0, h, 0.0, c, s, g, rcol, 0.0, 1000, &it, &rnorm, &which);
        bad += st != SBLAS_KRYLOV_CONVERGED || rnorm != 0.0 || it != 1 || c[0] != 1.0 || s[0] != 0.0 || g[0] != 2.0 || rcol[0] != 3.0;
    }
    // arguments
    {
        double one[2] = {1.0, 1.0};
        int64_t it = 0, which = 0, out[4], lower[12] = {0}, upper[12] = {0};
        double rnorm;
        bad += sblas_gmres_step_ref(-1, one, 1.0, one, one, one, one, 0.0, 1, &it, &rnorm, &which) != -1;
        bad += sblas_gmres_step_ref(M, one, 1.0, one, one, one, one, 0.0, 1, &it, &rnorm, &which) != -1;
        bad += sblas_gmres_step_ref(0, nullptr, 1.0, one, one, one, one, 0.0, 1, &it, &rnorm, &which) != -1;
        bad += sblas_gmres_solve_ref(-1, one, 1, one, one) != SBLAS_E_INVALID;
        bad += sblas_gmres_solve_ref(M + 1, one, M + 1, one, one) != SBLAS_E_INVALID;
        bad += sblas_gmres_solve_ref(2, one, 1, one, one) != SBLAS_E_INVALID;
        bad += sblas_gmres_solve_ref(1, nullptr, 1, one, one) != SBLAS_E_INVALID;
        lower[5] = 3, upper[5] = 7;
        bad += sblas_gmres_launches(30, SBLAS_PRECOND_NONE, nullptr, nullptr, out) != 30 * 9 + 3 + 4 || out[0] != 9 || out[1] != 3 || out[2] != 4 || out[3] != 6;
        bad += sblas_gmres_launches(5, SBLAS_PRECOND_JACOBI, lower, upper, out) != 5 * 9 + 3 + 4;
        bad += sblas_gmres_launches(1, SBLAS_PRECOND_ILU0, lower, upper, out) != 19 + 13 + 4 || out[0] != 19 || out[1] != 13;
        bad += sblas_gmres_launches(0, SBLAS_PRECOND_NONE, nullptr, nullptr, out) != -1;
        bad += sblas_gmres_launches(M + 1, SBLAS_PRECOND_NONE, nullptr, nullptr, out) != -1;
        bad += sblas_gmres_launches(30, 3, nullptr, nullptr, out) != -1;
        bad += sblas_gmres_launches(30, SBLAS_PRECOND_ILU0, nullptr, upper, out) != -1;
        bad += sblas_gmres_launches(30, SBLAS_PRECOND_ILU0, lower, nullptr, out) != -1;
        bad += sblas_gmres_launches(30, SBLAS_PRECOND_NONE, nullptr, nullptr, nullptr) != -1;
        lower[5] = -1;
        bad += sblas_gmres_launches(30, SBLAS_PRECOND_ILU0, lower, upper, out) != -1;
        // every kind (and the codes on either side), with each info missing, negative or good: an applied kind adds its
        // M^-1 to a step and to a close, ILU(0) from both infos and a cycle or a polynomial from the lower one alone
        for (int precond = -1; precond <= 5; ++precond)
            for (int lo = 0; lo < 3; ++lo)
                for (int up = 0; up < 3; ++up) {
                    lower[5] = lo == 1 ? -1 : 3, upper[5] = up == 1 ? -1 : 7;
                    const int64_t *li = lo ? lower : nullptr, *ui = up ? upper : nullptr;
                    const bool solves = precond == SBLAS_PRECOND_ILU0, single = precond == SBLAS_PRECOND_AMG || precond == SBLAS_PRECOND_CHEBYSHEV;
                    const bool refused = precond < 0 || precond > 4 || (solves && (lo != 2 || up != 2)) || (single && lo != 2);
                    const int64_t apply = solves ? 10 : single ? 3 : 0, got = sblas_gmres_launches(2, precond, li, ui, out);
                    if (refused) bad += got != -1;
                    else bad += got != 2 * (9 + apply) + (3 + apply) + 4 || out[0] != 9 + apply || out[1] != 3 + apply || out[2] != 4 || out[3] != 6;
                }
    }
    if (bad) printf("gmres rule check: %d FAILED\n", bad);
    else printf("gmres rule check: ok\n");
    return bad != 0;
}
