// amg_rule_check.cpp -- a stand-alone program over the AMG plan's host rule (s-blas_amd/csrc/amg_rule.cpp with ILU(0)'s
// structure check from ilu0_plan.cpp; no GPU, no HIP runtime), made to be built with a host sanitizer:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/amg_rule_check.cpp \
//       s-blas_amd/csrc/amg_rule.cpp s-blas_amd/csrc/ilu0_plan.cpp -o /tmp/amg_rule_check && /tmp/amg_rule_check
// It aggregates small matrices (n = 0 and 1, a diagonal, a tridiagonal, a grid, a clique, a star, an anisotropic grid
// with theta) out of arrays of exactly the sizes the contract names, so that a read or write past either end is the
// sanitizer's to find, checks every aggregate's invariants, builds the Galerkin hierarchy with a second, naive
// restatement of the COO order, runs the cycle reference on it against a restatement of the written order, and holds
// the launch counts against a hand count.  For smoothed aggregation it holds the coarsening guard against its expression,
// builds P (sblas_amg_prolongator_ref, counted first and then written into arrays of exactly that size), R = P^T and the two
// products in a naive restatement of the pinned orders, and runs sblas_amg_transfer_ref and sblas_amg_cycle_sa_ref
// against the written order once more, n = 0 and 1 included.  For the device aggregation it runs the rule in
// synchronous rounds (sblas_amg_roots_rounds_ref) on the same matrices with a root array of exactly n bytes and holds its
// roots against sblas_amg_aggregate's.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <vector>
#include "../include/sblas_hip.h"

#pragma clang fp contract(off)

struct Csr {
    int64_t n = 0;
    std::vector<int32_t> rowptr{0}, colidx;
    std::vector<double> val;
    void row(const std::map<int32_t, double> &r)
    {
        for (const auto &kv : r) colidx.push_back(kv.first), val.push_back(kv.second);
        rowptr.push_back((int32_t)colidx.size());
        ++n;
    }
};

static Csr grid(int side, double ax, double ay)
{
    Csr a;
    for (int y = 0; y < side; ++y)
        for (int x = 0; x < side; ++x) {
            std::map<int32_t, double> r;
            r[y * side + x] = 2 * ax + 2 * ay;
            if (x > 0) r[y * side + x - 1] = -ax;
            if (x + 1 < side) r[y * side + x + 1] = -ax;
            if (y > 0) r[(y - 1) * side + x] = -ay;
            if (y + 1 < side) r[(y + 1) * side + x] = -ay;
            a.row(r);
        }
    return a;
}

struct Level {
    Csr a;
    std::vector<double> wd;
    std::vector<int32_t> agg, aggptr, members;
};

static int bad = 0;
static void expect(bool ok, const char *what)
{
    if (!ok) ++bad, fprintf(stderr, "amg_rule_check: %s\n", what);
}

// one level's aggregation out of exact-size arrays, with its invariants
static int64_t aggregate(const Csr &a, double theta, uint32_t seed, uint32_t level, Level &out)
{
    const int64_t n = a.n;
    std::vector<int32_t> agg((size_t)n), members((size_t)n), aggptr((size_t)n + 1);
    int64_t n_agg = -1, row = 0;
    const int rc = sblas_amg_aggregate(n, a.rowptr.data(), a.colidx.data(), theta > 0 ? a.val.data() : nullptr, theta, seed, level, agg.data(),
                                       aggptr.data(), members.data(), &n_agg, &row);
    expect(rc == SBLAS_OK && row == -1 && n_agg >= 0 && n_agg <= n, "aggregate accepts a sound structure");
    aggptr.resize((size_t)n_agg + 1);
    expect(aggptr[0] == 0 && aggptr[(size_t)n_agg] == n, "aggptr spans the vertices");
    std::vector<int> seen((size_t)n, 0);
    for (int64_t g = 0; g < n_agg; ++g)
        for (int32_t k = aggptr[(size_t)g]; k < aggptr[(size_t)g + 1]; ++k) {
            expect(agg[(size_t)members[(size_t)k]] == g, "a member lies in its aggregate");
            expect(k == aggptr[(size_t)g] || members[(size_t)k] > members[(size_t)k - 1], "members ascend inside an aggregate");
            ++seen[(size_t)members[(size_t)k]];
        }
    for (int64_t v = 0; v < n; ++v) expect(seen[(size_t)v] == 1, "every vertex is in exactly one aggregate");
    out.agg = agg, out.aggptr = aggptr, out.members = members;
    return n_agg;
}

// the triplets (agg[row], agg[col]) in stored order, sorted by (row, col) with equal pairs in input order, summed left to right
static Csr galerkin(const Csr &a, const std::vector<int32_t> &agg, int64_t nc)
{
    std::vector<size_t> order(a.colidx.size());
    std::vector<int32_t> tr(order.size()), tc(order.size());
    for (int64_t i = 0; i < a.n; ++i)
        for (int32_t e = a.rowptr[(size_t)i]; e < a.rowptr[(size_t)i + 1]; ++e) tr[(size_t)e] = agg[(size_t)i], tc[(size_t)e] = agg[(size_t)a.colidx[(size_t)e]];
    for (size_t k = 0; k < order.size(); ++k) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return tr[x] != tr[y] ? tr[x] < tr[y] : tc[x] < tc[y]; });
    Csr c;
    c.n = nc;
    c.rowptr.assign((size_t)nc + 1, 0);
    for (size_t k = 0; k < order.size(); ++k) {
        const size_t e = order[k];
        if (k > 0 && tr[e] == tr[order[k - 1]] && tc[e] == tc[order[k - 1]]) {
            c.val.back() = c.val.back() + a.val[e];
        } else {
            c.colidx.push_back(tc[e]), c.val.push_back(a.val[e]);
            ++c.rowptr[(size_t)tr[e] + 1];
        }
    }
    for (int64_t g = 0; g < nc; ++g) c.rowptr[(size_t)g + 1] += c.rowptr[(size_t)g];
    return c;
}

static std::vector<Level> hierarchy(const Csr &a, double theta, int64_t coarse_max, int smoother, double omega)
{
    std::vector<Level> lv;
    if (a.n == 0) return lv;
    Csr cur = a;
    for (;;) {
        Level L;
        L.a = cur;
        L.wd.resize((size_t)cur.n);
        int64_t row = 0;
        expect(sblas_amg_wd_ref(cur.n, cur.rowptr.data(), cur.colidx.data(), cur.val.data(), smoother, omega, L.wd.data(), &row) == SBLAS_OK && row == -1,
               "wd of a sound level");
        const bool coarsen = cur.n > coarse_max && lv.size() + 1 < 20;
        int64_t nc = cur.n;
        if (coarsen) nc = aggregate(cur, theta, 0, (uint32_t)lv.size(), L);
        if (nc >= cur.n) L.agg.clear(), L.aggptr.clear(), L.members.clear();
        lv.push_back(L);
        if (nc >= cur.n) return lv;
        cur = galerkin(cur, lv.back().agg, nc);
    }
}

// the written order once more
static double row_sum(const Csr &a, int64_t i, const std::vector<double> &x)
{
    const int p = a.rowptr[(size_t)i + 1] - a.rowptr[(size_t)i], G = p <= 4 ? 4 : p <= 32 ? 16 : 64;
    std::vector<double> v((size_t)G, 0.0), w((size_t)G);
    for (int l = 0; l < G; ++l)
        for (int e = a.rowptr[(size_t)i] + l; e < a.rowptr[(size_t)i + 1]; e += G) v[(size_t)l] = fma(a.val[(size_t)e], x[(size_t)a.colidx[(size_t)e]], v[(size_t)l]);
    for (int m = 1; m < G; m <<= 1) {
        for (int l = 0; l < G; ++l) w[(size_t)l] = v[(size_t)l] + v[(size_t)(l ^ m)];
        v = w;
    }
    return v[0];
}

static std::vector<double> sweep(const Level &L, const std::vector<double> &b, const std::vector<double> &x, bool residual)
{
    std::vector<double> y((size_t)L.a.n);
    for (int64_t i = 0; i < L.a.n; ++i) {
        const double d = b[(size_t)i] - row_sum(L.a, i, x), t = L.wd[(size_t)i] * d;
        y[(size_t)i] = residual ? d : x[(size_t)i] + t;
    }
    return y;
}

static std::vector<double> cycle(const std::vector<Level> &lv, size_t l, const std::vector<double> &b, int nu, int cs, double scale)
{
    const Level &L = lv[l];
    std::vector<double> x((size_t)L.a.n);
    for (int64_t i = 0; i < L.a.n; ++i) x[(size_t)i] = L.wd[(size_t)i] * b[(size_t)i];
    if (l + 1 == lv.size()) {
        for (int k = 1; k < cs; ++k) x = sweep(L, b, x, false);
        return x;
    }
    for (int k = 1; k < nu; ++k) x = sweep(L, b, x, false);
    const std::vector<double> res = sweep(L, b, x, true);
    std::vector<double> bc(L.aggptr.size() - 1);
    for (size_t g = 0; g + 1 < L.aggptr.size(); ++g) {
        double s = 0.0;
        for (int32_t k = L.aggptr[g]; k < L.aggptr[g + 1]; ++k) s = s + res[(size_t)L.members[(size_t)k]];
        bc[g] = s;
    }
    const std::vector<double> e = cycle(lv, l + 1, bc, nu, cs, scale);
    for (int64_t i = 0; i < L.a.n; ++i) {
        const double t = scale * e[(size_t)L.agg[(size_t)i]];
        x[(size_t)i] = x[(size_t)i] + t;
    }
    for (int k = 0; k < nu; ++k) x = sweep(L, b, x, false);
    return x;
}

static void check_case(const char *name, const Csr &a, double theta, int64_t coarse_max, size_t want_levels)
{
    for (int smoother = 0; smoother < 2; ++smoother)
        for (int nu = 1; nu <= 2; ++nu) {
            const double omega = smoother ? 1.0 : 2.0 / 3.0, scale = nu == 1 ? 1.0 : 1.5;
            const std::vector<Level> lv = hierarchy(a, theta, coarse_max, smoother, omega);
            if (want_levels) expect(lv.size() == want_levels, name);
            const int k = (int)lv.size();
            std::vector<int64_t> n;
            std::vector<const int32_t *> rp, ci, agg, aggptr, members;
            std::vector<const double *> val, wd;
            for (const Level &L : lv) {
                n.push_back(L.a.n), rp.push_back(L.a.rowptr.data()), ci.push_back(L.a.colidx.data()), val.push_back(L.a.val.data());
                wd.push_back(L.wd.data()), agg.push_back(L.agg.data()), aggptr.push_back(L.aggptr.data()), members.push_back(L.members.data());
            }
            std::vector<double> r((size_t)a.n), z((size_t)a.n, -7.0);
            for (size_t i = 0; i < r.size(); ++i) r[i] = sin(1.0 + (double)i) + 0.25;
            const int rc = sblas_amg_cycle_ref(k, n.data(), rp.data(), ci.data(), val.data(), wd.data(), agg.data(), aggptr.data(), members.data(), nu,
                                               3, scale, r.data(), z.data());
            expect(rc == SBLAS_OK, "cycle_ref accepts a sound hierarchy");
            if (k > 0) {
                const std::vector<double> want = cycle(lv, 0, r, nu, 3, scale);
                expect(memcmp(want.data(), z.data(), z.size() * 8) == 0, name);
                expect(sblas_amg_cycle_ref(k, n.data(), rp.data(), ci.data(), val.data(), wd.data(), agg.data(), aggptr.data(), members.data(), nu, 3,
                                           scale, r.data(), r.data()) == SBLAS_E_INVALID,
                       "z must not be r");
            }
            expect(sblas_amg_launches(k, nu, 3) == (k == 0 ? 0 : (int64_t)(k - 1) * (2 * nu + 3) + 3), "launches of a cycle");
        }
}

// ---- smoothed aggregation ----
typedef std::vector<std::vector<std::pair<int32_t, double>>> Rows; // every row's (column, value) in the pinned numbering

// sorted by column, equal columns in input order, each run added left to right
static Csr sum_rows(const Rows &rows)
{
    Csr c;
    for (const auto &r : rows) {
        std::vector<std::pair<int32_t, double>> s(r);
        std::stable_sort(s.begin(), s.end(), [](const std::pair<int32_t, double> &x, const std::pair<int32_t, double> &y) { return x.first < y.first; });
        for (size_t k = 0; k < s.size(); ++k) {
            if (k > 0 && s[k].first == s[k - 1].first) c.val.back() = c.val.back() + s[k].second;
            else c.colidx.push_back(s[k].first), c.val.push_back(s[k].second);
        }
        c.rowptr.push_back((int32_t)c.colidx.size());
        ++c.n;
    }
    return c;
}

static Csr product(const Csr &a, const Csr &b)
{
    Rows rows((size_t)a.n);
    for (int64_t i = 0; i < a.n; ++i)
        for (int32_t e = a.rowptr[(size_t)i]; e < a.rowptr[(size_t)i + 1]; ++e)
            for (int32_t f = b.rowptr[(size_t)a.colidx[(size_t)e]]; f < b.rowptr[(size_t)a.colidx[(size_t)e] + 1]; ++f)
                rows[(size_t)i].emplace_back(b.colidx[(size_t)f], a.val[(size_t)e] * b.val[(size_t)f]);
    return sum_rows(rows);
}

static Csr transpose(const Csr &p, int64_t cols)
{
    Rows rows((size_t)cols);
    for (int64_t i = 0; i < p.n; ++i)
        for (int32_t e = p.rowptr[(size_t)i]; e < p.rowptr[(size_t)i + 1]; ++e) rows[(size_t)p.colidx[(size_t)e]].emplace_back((int32_t)i, p.val[(size_t)e]);
    return sum_rows(rows); // rows ascend already and no pair repeats: nothing is added
}

struct SaLevel {
    Csr a, p, r;
    std::vector<double> wd;
};

static Csr prolongator(const Csr &a, const std::vector<int32_t> &agg, int64_t nc, double omega_p)
{
    // the library's, counted first, then written into arrays of exactly that size
    std::vector<int32_t> prp((size_t)a.n + 1);
    int64_t count = -1, row = 0;
    expect(sblas_amg_prolongator_ref(a.n, a.rowptr.data(), a.colidx.data(), a.val.data(), agg.data(), nc, omega_p, prp.data(), nullptr, nullptr, &count,
                                     &row) == SBLAS_OK && row == -1 && count >= a.n,
           "prolongator_ref counts");
    Csr p;
    p.n = a.n, p.rowptr.assign((size_t)a.n + 1, 0), p.colidx.resize((size_t)count), p.val.resize((size_t)count);
    int64_t again = -1;
    expect(sblas_amg_prolongator_ref(a.n, a.rowptr.data(), a.colidx.data(), a.val.data(), agg.data(), nc, omega_p, p.rowptr.data(), p.colidx.data(),
                                     p.val.data(), &again, &row) == SBLAS_OK && again == count,
           "prolongator_ref writes what it counted");
    // the rule once more
    Rows rows((size_t)a.n);
    for (int64_t i = 0; i < a.n; ++i) {
        double d = 0.0;
        for (int32_t e = a.rowptr[(size_t)i]; e < a.rowptr[(size_t)i + 1]; ++e)
            if (a.colidx[(size_t)e] == i) d = a.val[(size_t)e];
        const double q = omega_p / d;
        for (int32_t e = a.rowptr[(size_t)i]; e < a.rowptr[(size_t)i + 1]; ++e) {
            const double prod = q * a.val[(size_t)e];
            rows[(size_t)i].emplace_back(agg[(size_t)a.colidx[(size_t)e]], a.colidx[(size_t)e] == i ? 1.0 - prod : -prod);
        }
    }
    const Csr want = sum_rows(rows);
    expect(want.rowptr == p.rowptr && want.colidx == p.colidx && want.val.size() == p.val.size() &&
               (p.val.empty() || memcmp(want.val.data(), p.val.data(), p.val.size() * 8) == 0),
           "prolongator_ref has the rule's bits");
    return p;
}

static std::vector<double> transfer(const Csr &m, const std::vector<double> &in)
{
    std::vector<double> s((size_t)m.n);
    for (int64_t i = 0; i < m.n; ++i) s[(size_t)i] = row_sum(m, i, in);
    return s;
}

static std::vector<double> cycle_sa(const std::vector<SaLevel> &lv, size_t l, const std::vector<double> &b, int nu, int cs, double scale)
{
    Level L;
    L.a = lv[l].a, L.wd = lv[l].wd;
    std::vector<double> x((size_t)L.a.n);
    for (int64_t i = 0; i < L.a.n; ++i) x[(size_t)i] = L.wd[(size_t)i] * b[(size_t)i];
    if (l + 1 == lv.size()) {
        for (int k = 1; k < cs; ++k) x = sweep(L, b, x, false);
        return x;
    }
    for (int k = 1; k < nu; ++k) x = sweep(L, b, x, false);
    const std::vector<double> e = cycle_sa(lv, l + 1, transfer(lv[l].r, sweep(L, b, x, true)), nu, cs, scale);
    const std::vector<double> pe = transfer(lv[l].p, e);
    for (int64_t i = 0; i < L.a.n; ++i) {
        const double t = scale * pe[(size_t)i];
        x[(size_t)i] = x[(size_t)i] + t;
    }
    for (int k = 0; k < nu; ++k) x = sweep(L, b, x, false);
    return x;
}

static void check_smoothed(const char *name, const Csr &a, double theta, int64_t coarse_max, double min_reduction, size_t want_levels)
{
    std::vector<SaLevel> lv;
    Csr cur = a;
    while (a.n > 0) {
        SaLevel S;
        S.a = cur;
        S.wd.resize((size_t)cur.n);
        int64_t row = 0;
        expect(sblas_amg_wd_ref(cur.n, cur.rowptr.data(), cur.colidx.data(), cur.val.data(), SBLAS_AMG_JACOBI, 2.0 / 3.0, S.wd.data(), &row) == SBLAS_OK,
               "wd of a smoothed level");
        Level L;
        int64_t nc = cur.n;
        if (cur.n > coarse_max && lv.size() + 1 < 20) nc = aggregate(cur, theta, 0, (uint32_t)lv.size(), L);
        const int keep = sblas_amg_keep_level(cur.n, nc, min_reduction);
        expect(keep == (nc < cur.n && (double)nc <= (1.0 - min_reduction) * (double)cur.n ? 1 : 0), "keep_level is its expression");
        if (!keep) {
            lv.push_back(S);
            break;
        }
        S.p = prolongator(cur, L.agg, nc, 2.0 / 3.0);
        S.r = transpose(S.p, nc);
        lv.push_back(S);
        cur = product(S.r, product(cur, S.p));
    }
    if (want_levels) expect(lv.size() == want_levels, name);
    const int k = (int)lv.size();
    std::vector<int64_t> n;
    std::vector<const int32_t *> rp, ci, prp, pci, rrp, rci;
    std::vector<const double *> val, wd, pv, rv;
    for (const SaLevel &S : lv) {
        n.push_back(S.a.n), rp.push_back(S.a.rowptr.data()), ci.push_back(S.a.colidx.data()), val.push_back(S.a.val.data()), wd.push_back(S.wd.data());
        prp.push_back(S.p.rowptr.data()), pci.push_back(S.p.colidx.data()), pv.push_back(S.p.val.data());
        rrp.push_back(S.r.rowptr.data()), rci.push_back(S.r.colidx.data()), rv.push_back(S.r.val.data());
    }
    std::vector<double> r((size_t)a.n), z((size_t)a.n, -7.0);
    for (size_t i = 0; i < r.size(); ++i) r[i] = sin(1.0 + (double)i) + 0.25;
    for (int nu = 1; nu <= 2; ++nu) {
        const double scale = nu == 1 ? 1.0 : 1.5;
        expect(sblas_amg_cycle_sa_ref(k, n.data(), rp.data(), ci.data(), val.data(), wd.data(), prp.data(), pci.data(), pv.data(), rrp.data(), rci.data(),
                                      rv.data(), nu, 3, scale, r.data(), z.data()) == SBLAS_OK,
               "cycle_sa_ref accepts a sound hierarchy");
        if (k > 0) {
            const std::vector<double> want = cycle_sa(lv, 0, r, nu, 3, scale);
            expect(memcmp(want.data(), z.data(), z.size() * 8) == 0, name);
            expect(sblas_amg_cycle_sa_ref(k, n.data(), rp.data(), ci.data(), val.data(), wd.data(), prp.data(), pci.data(), pv.data(), rrp.data(),
                                          rci.data(), rv.data(), nu, 3, scale, r.data(), r.data()) == SBLAS_E_INVALID,
                   "z must not be r");
        }
    }
    for (size_t l = 0; l + 1 < lv.size(); ++l) { // the transfers alone, out of exact-size arrays
        const SaLevel &S = lv[l];
        std::vector<double> res((size_t)S.a.n), e((size_t)S.r.n), bc((size_t)S.r.n, -7.0), x((size_t)S.a.n);
        for (size_t i = 0; i < res.size(); ++i) res[i] = cos(2.0 + (double)i), x[i] = 0.5 - (double)(i % 5);
        for (size_t i = 0; i < e.size(); ++i) e[i] = sin(3.0 + (double)i);
        expect(sblas_amg_transfer_ref(SBLAS_AMG_RESTRICT, S.r.n, S.r.rowptr.data(), S.r.colidx.data(), S.r.val.data(), 0.0, res.data(), bc.data()) == SBLAS_OK,
               "transfer_ref restricts");
        const std::vector<double> want_bc = transfer(S.r, res), pe = transfer(S.p, e);
        expect(memcmp(want_bc.data(), bc.data(), bc.size() * 8) == 0, "the restriction's bits");
        std::vector<double> want_x(x);
        for (size_t i = 0; i < x.size(); ++i) {
            const double t = 1.5 * pe[i];
            want_x[i] = x[i] + t;
        }
        expect(sblas_amg_transfer_ref(SBLAS_AMG_PROLONG, S.a.n, S.p.rowptr.data(), S.p.colidx.data(), S.p.val.data(), 1.5, e.data(), x.data()) == SBLAS_OK,
               "transfer_ref prolongs");
        expect(memcmp(want_x.data(), x.data(), x.size() * 8) == 0, "the prolongation's bits");
    }
}

// the rule in synchronous rounds out of exact-size arrays: its roots are the greedy walk's, numbered in ascending order
static void check_rounds(const char *name, const Csr &a, double theta)
{
    const int64_t n = a.n;
    const uint32_t salts[3][2] = {{0, 0}, {7, 0}, {0, 3}};
    for (const auto &sl : salts) {
        Level L;
        const int64_t n_agg = aggregate(a, theta, sl[0], sl[1], L);
        std::vector<unsigned char> root((size_t)n, 2);
        int64_t rounds = -1, row = 0;
        const int rc = sblas_amg_roots_rounds_ref(n, a.rowptr.data(), a.colidx.data(), theta > 0 ? a.val.data() : nullptr, theta, sl[0], sl[1],
                                                  root.data(), &rounds, &row);
        expect(rc == SBLAS_OK && row == -1, name);
        expect(n == 0 ? rounds == 0 : (rounds >= 1 && rounds <= n), "the rounds that decided a vertex: one at least, n at most");
        int64_t k = 0;
        for (int64_t v = 0; v < n; ++v) {
            expect(root[(size_t)v] <= 1, "every vertex is decided");
            if (root[(size_t)v] == 1) expect(L.agg[(size_t)v] == k++, "the roots carry the aggregates' numbers in ascending order");
        }
        expect(k == n_agg, "one root an aggregate");
    }
}

int main()
{
    int64_t lim[8];
    expect(sblas_amg_limits(lim) == SBLAS_OK && sblas_amg_limits(nullptr) == SBLAS_E_INVALID, "limits");
    expect(lim[0] == 4 && lim[1] == 32 && lim[3] == 64 && lim[4] == 20 && lim[5] == 1 && lim[6] == 8, "the defaults");
    expect(sblas_amg_launches(4, 1, 8) == 23 && sblas_amg_launches(1, 1, 8) == 8 && sblas_amg_launches(0, 1, 8) == 0, "launch counts");
    expect(sblas_amg_launches(-1, 1, 8) == -1 && sblas_amg_launches(3, 0, 8) == -1 && sblas_amg_launches(3, 1, 0) == -1, "launch refusals");

    Csr empty, one, diag, tri, clique, star;
    one.row({{0, 2.0}});
    for (int i = 0; i < 40; ++i) diag.row({{i, 1.0 + i % 3}});
    for (int i = 0; i < 300; ++i) {
        std::map<int32_t, double> r{{i, 2.0}};
        if (i > 0) r[i - 1] = -1.0;
        if (i + 1 < 300) r[i + 1] = -1.0;
        tri.row(r);
    }
    for (int i = 0; i < 70; ++i) {
        std::map<int32_t, double> r;
        for (int j = 0; j < 70; ++j) r[j] = i == j ? 71.0 : -1.0;
        clique.row(r);
    }
    {
        std::map<int32_t, double> hub;
        for (int j = 0; j < 200; ++j) hub[j] = j ? -1.0 : 200.0;
        star.row(hub);
        for (int i = 1; i < 200; ++i) star.row({{0, -1.0}, {i, 2.0}});
    }
    check_case("n = 0", empty, 0.0, 64, 0);
    check_case("n = 1", one, 0.0, 64, 1);
    check_case("diagonal: one level", diag, 0.0, 8, 1);
    check_case("tridiagonal", tri, 0.0, 16, 0);
    check_case("grid", grid(12, 1.0, 1.0), 0.0, 16, 0);
    check_case("clique", clique, 0.0, 16, 2);
    check_case("star", star, 0.0, 64, 0);
    check_case("anisotropic grid", grid(10, 1.0, 0.01), 0.25, 16, 0);

    // smoothed aggregation: the same matrices; the star stays one level under the guard and loses a vertex a level without
    check_smoothed("smoothed n = 0", empty, 0.0, 64, 0.2, 0);
    check_smoothed("smoothed n = 1", one, 0.0, 64, 0.2, 1);
    check_smoothed("smoothed diagonal: one level", diag, 0.0, 8, 0.2, 1);
    check_smoothed("smoothed tridiagonal", tri, 0.0, 16, 0.2, 0);
    check_smoothed("smoothed grid", grid(12, 1.0, 1.0), 0.0, 16, 0.2, 0);
    check_smoothed("smoothed clique", clique, 0.0, 16, 0.0, 2);
    check_smoothed("smoothed star, guarded", star, 0.0, 64, 0.2, 1);
    check_smoothed("smoothed anisotropic grid", grid(10, 1.0, 0.01), 0.25, 16, 0.2, 0);
    {
        expect(sblas_amg_keep_level(10, 8, 0.2) == 1 && sblas_amg_keep_level(10, 9, 0.2) == 0 && sblas_amg_keep_level(10, 9, 0.0) == 1 &&
                   sblas_amg_keep_level(10, 10, 0.0) == 0 && sblas_amg_keep_level(0, 0, 0.0) == 0,
               "keep_level at its boundaries");
        expect(sblas_amg_keep_level(-1, 0, 0.0) == -1 && sblas_amg_keep_level(4, -1, 0.0) == -1 && sblas_amg_keep_level(4, 2, 1.0) == -1 &&
                   sblas_amg_keep_level(4, 2, -0.5) == -1 && sblas_amg_keep_level(4, 2, NAN) == -1,
               "keep_level refusals");
        Csr g = grid(4, 1.0, 1.0);
        std::vector<int32_t> agg(16, 0), prp(17);
        int64_t count = 0, row = -1;
        const double omegas[4] = {0.0, -1.0, NAN, INFINITY};
        for (double w : omegas)
            expect(sblas_amg_prolongator_ref(16, g.rowptr.data(), g.colidx.data(), g.val.data(), agg.data(), 1, w, prp.data(), nullptr, nullptr, &count, &row) ==
                       SBLAS_E_INVALID,
                   "omega_P must be finite and > 0");
        agg[7] = 1;
        expect(sblas_amg_prolongator_ref(16, g.rowptr.data(), g.colidx.data(), g.val.data(), agg.data(), 1, 0.5, prp.data(), nullptr, nullptr, &count, &row) ==
                   SBLAS_E_INVALID,
               "an aggregate beyond n_agg");
        agg[7] = 0;
        for (int32_t e = g.rowptr[9]; e < g.rowptr[10]; ++e)
            if (g.colidx[(size_t)e] == 9) g.colidx[(size_t)e] = 8;
        expect(sblas_amg_prolongator_ref(16, g.rowptr.data(), g.colidx.data(), g.val.data(), agg.data(), 1, 0.5, prp.data(), nullptr, nullptr, &count, &row) ==
                       SBLAS_E_INVALID && row == 9,
               "a missing diagonal is named");
        std::vector<double> v(16, 1.0);
        expect(sblas_amg_transfer_ref(2, 16, g.rowptr.data(), g.colidx.data(), g.val.data(), 1.0, v.data(), v.data()) == SBLAS_E_INVALID &&
                   sblas_amg_transfer_ref(SBLAS_AMG_RESTRICT, 16, g.rowptr.data(), g.colidx.data(), g.val.data(), 1.0, v.data(), v.data()) == SBLAS_E_INVALID,
               "transfer_ref refusals");
    }

    // refusals, each with its row
    {
        Csr g = grid(4, 1.0, 1.0);
        std::vector<int32_t> agg(16), ptr(17), mem(16);
        int64_t n_agg = 0, row = -1;
        std::swap(g.colidx[(size_t)g.rowptr[5]], g.colidx[(size_t)g.rowptr[5] + 1]); // row 5 no longer ascends
        expect(sblas_amg_aggregate(16, g.rowptr.data(), g.colidx.data(), nullptr, 0.0, 0, 0, agg.data(), ptr.data(), mem.data(), &n_agg, &row) ==
                       SBLAS_E_INVALID && row == 5,
               "an unsorted row is named");
        g = grid(4, 1.0, 1.0);
        for (int32_t e = g.rowptr[9]; e < g.rowptr[10]; ++e)
            if (g.colidx[(size_t)e] == 9) g.colidx[(size_t)e] = 8; // row 9 loses its diagonal (and doubles a column)
        expect(sblas_amg_aggregate(16, g.rowptr.data(), g.colidx.data(), nullptr, 0.0, 0, 0, agg.data(), ptr.data(), mem.data(), &n_agg, &row) ==
                       SBLAS_E_INVALID && row == 9,
               "a missing diagonal is named");
        g = grid(4, 1.0, 1.0);
        const double thetas[3] = {-0.5, 1.5, NAN};
        for (double t : thetas)
            expect(sblas_amg_aggregate(16, g.rowptr.data(), g.colidx.data(), g.val.data(), t, 0, 0, agg.data(), ptr.data(), mem.data(), &n_agg, &row) ==
                       SBLAS_E_INVALID,
                   "theta outside [0, 1]");
        expect(sblas_amg_aggregate(16, g.rowptr.data(), g.colidx.data(), nullptr, 0.25, 0, 0, agg.data(), ptr.data(), mem.data(), &n_agg, &row) ==
                   SBLAS_E_INVALID,
               "theta > 0 without values");
        std::vector<double> wd(16);
        for (int32_t e = g.rowptr[7]; e < g.rowptr[8]; ++e)
            if (g.colidx[(size_t)e] == 7) g.val[(size_t)e] = 0.0;
        expect(sblas_amg_wd_ref(16, g.rowptr.data(), g.colidx.data(), g.val.data(), SBLAS_AMG_JACOBI, 0.5, wd.data(), &row) == SBLAS_OK && row == 7,
               "a zero diagonal is reported");
    }
    // the rule in synchronous rounds: the same matrices, and its refusals
    check_rounds("rounds n = 0", empty, 0.0);
    check_rounds("rounds n = 1", one, 0.0);
    check_rounds("rounds diagonal", diag, 0.0);
    check_rounds("rounds tridiagonal", tri, 0.0);
    check_rounds("rounds grid", grid(12, 1.0, 1.0), 0.0);
    check_rounds("rounds clique", clique, 0.0);
    check_rounds("rounds star", star, 0.0);
    check_rounds("rounds anisotropic grid", grid(10, 1.0, 0.01), 0.25);
    check_rounds("rounds anisotropic grid, theta 1", grid(10, 1.0, 0.01), 1.0);
    {
        Csr g = grid(4, 1.0, 1.0);
        std::vector<unsigned char> root(16);
        int64_t rounds = 0, row = -1;
        expect(sblas_amg_roots_rounds_ref(16, g.rowptr.data(), g.colidx.data(), g.val.data(), NAN, 0, 0, root.data(), &rounds, &row) == SBLAS_E_INVALID &&
                   sblas_amg_roots_rounds_ref(16, g.rowptr.data(), g.colidx.data(), nullptr, 0.25, 0, 0, root.data(), &rounds, &row) == SBLAS_E_INVALID &&
                   sblas_amg_roots_rounds_ref(16, g.rowptr.data(), g.colidx.data(), nullptr, 0.0, 0, 0, nullptr, &rounds, &row) == SBLAS_E_INVALID &&
                   sblas_amg_roots_rounds_ref(16, g.rowptr.data(), g.colidx.data(), nullptr, 0.0, 0, 0, root.data(), nullptr, &row) == SBLAS_E_INVALID,
               "rounds_ref refusals");
        std::swap(g.colidx[(size_t)g.rowptr[5]], g.colidx[(size_t)g.rowptr[5] + 1]);
        expect(sblas_amg_roots_rounds_ref(16, g.rowptr.data(), g.colidx.data(), nullptr, 0.0, 0, 0, root.data(), &rounds, &row) == SBLAS_E_INVALID && row == 5,
               "rounds_ref names an unsorted row");
    }
    if (bad) return fprintf(stderr, "amg_rule_check: %d failures\n", bad), 1;
    printf("amg_rule_check: ok\n");
    return 0;
}
