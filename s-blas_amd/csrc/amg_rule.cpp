// amg_rule.cpp -- the host rule of the aggregation AMG plan (amg.hip): the pinned aggregation of one
// level, the smoother's diagonal, the launch count and the whole V-cycle restated in plain C++.  Pure functions of host
// arrays; no GPU call in this file, so it is testable on a CPU box (and under a host sanitizer).
// For smoothed aggregation it also holds the coarsening guard, the prolongator P in the pinned order (the
// COO sum of (row(e), agg[col(e)], t_e)), the transfers' row product in lane order and the walk with general P and R.
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <utility>
#include <vector>
#include "../../include/sblas_hip.h"
#include "amg.h"
#include "amg_multi.h"
#include "color.h"

#pragma clang fp contract(off) // every product and sum below is rounded on its own; the row sums call fma() by name

namespace sblas {

// theta * max_{k != i} |a_ik|, the product rounded: the maximum by `a > m` from m = 0, so a NaN entry is never the
// maximum (and, through |a| >= bound, never strong); a row with no off-diagonal entry has bound 0
void amg_strength_bounds(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, double theta, std::vector<double> &bound)
{
    bound.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        double m = 0.0;
        for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
            const double a = fabs(val[e]);
            if (colidx[e] != i && a > m) m = a;
        }
        bound[(size_t)i] = theta * m;
    }
}

int64_t amg_aggregate(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, double theta, uint32_t seed,
                      uint32_t level, int32_t *agg, std::vector<int32_t> &aggptr, int32_t *members)
{
    const bool by_value = val != nullptr && theta > 0.0;
    // strong(i, e): entry e of row i is a strong off-diagonal one.  Only row i's own entries are consulted.
    std::vector<double> bound;
    if (by_value) amg_strength_bounds(n, rowptr, colidx, val, theta, bound);
    const auto strong = [&](int64_t i, int64_t e) { return colidx[e] != i && (!by_value || fabs(val[e]) >= bound[(size_t)i]); };

    // roots: the greedy maximal independent set in descending priority (no two vertices tie)
    const uint32_t salt = color_salt(seed + level);
    std::vector<int32_t> order((size_t)n);
    for (int64_t v = 0; v < n; ++v) order[(size_t)v] = (int32_t)v;
    std::sort(order.begin(), order.end(),
              [&](int32_t a, int32_t b) { return color_priority((uint32_t)a, salt) > color_priority((uint32_t)b, salt); });
    std::vector<char> root((size_t)n, 0);
    for (int64_t k = 0; k < n; ++k) {
        const int32_t v = order[(size_t)k];
        bool free_of_roots = true;
        for (int64_t e = rowptr[v]; e < rowptr[v + 1] && free_of_roots; ++e)
            if (strong(v, e) && root[(size_t)colidx[e]]) free_of_roots = false;
        root[(size_t)v] = free_of_roots;
    }
    // aggregates: roots numbered in ascending vertex index; every other vertex joins the first root among its strong
    // neighbours in stored order (it has one: otherwise it would be a root)
    int64_t n_agg = 0;
    for (int64_t v = 0; v < n; ++v) agg[v] = root[(size_t)v] ? (int32_t)n_agg++ : -1;
    for (int64_t v = 0; v < n; ++v) {
        if (root[(size_t)v]) continue;
        for (int64_t e = rowptr[v]; e < rowptr[v + 1]; ++e)
            if (strong(v, e) && root[(size_t)colidx[e]]) {
                agg[v] = agg[colidx[e]];
                break;
            }
    }
    // members: the vertices by (aggregate, vertex), a counting sort stable in the vertex
    aggptr.assign((size_t)n_agg + 1, 0);
    for (int64_t v = 0; v < n; ++v) ++aggptr[(size_t)agg[v] + 1];
    for (int64_t a = 0; a < n_agg; ++a) aggptr[(size_t)a + 1] += aggptr[(size_t)a];
    std::vector<int32_t> fill(aggptr.begin(), aggptr.end() - 1);
    for (int64_t v = 0; v < n; ++v) members[fill[(size_t)agg[v]]++] = (int32_t)v;
    return n_agg;
}

int64_t amg_roots_rounds(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, double theta, uint32_t seed, uint32_t level,
                         unsigned char *root)
{
    const bool by_value = val != nullptr && theta > 0.0;
    std::vector<double> bound;
    if (by_value) amg_strength_bounds(n, rowptr, colidx, val, theta, bound);
    const uint32_t salt = color_salt(seed + level);
    std::vector<int8_t> state((size_t)n, -1); // -1 undecided, 0 non-root, 1 root: final once written
    std::vector<int32_t> open((size_t)n), still;
    std::vector<std::pair<int32_t, int8_t>> decided;
    for (int64_t v = 0; v < n; ++v) open[(size_t)v] = (int32_t)v;
    int64_t rounds = 0;
    while (!open.empty()) {
        decided.clear(), still.clear();
        for (const int32_t v : open) { // reads only the states of the rounds before this one
            const uint32_t hv = color_priority((uint32_t)v, salt);
            bool non_root = false, wait = false;
            for (int64_t e = rowptr[v]; e < rowptr[v + 1] && !non_root; ++e) {
                const int32_t u = colidx[e];
                if (u == v || (by_value && !(fabs(val[e]) >= bound[(size_t)v])) || !(color_priority((uint32_t)u, salt) > hv)) continue;
                if (state[(size_t)u] == 1) non_root = true;
                else if (state[(size_t)u] < 0) wait = true;
            }
            if (non_root || !wait) decided.emplace_back(v, non_root ? 0 : 1);
            else still.push_back(v);
        }
        if (decided.empty()) return -1; // cannot happen: the open vertex of greatest priority waits for nobody
        for (const auto &d : decided) state[(size_t)d.first] = d.second;
        open.swap(still);
        ++rounds;
    }
    for (int64_t v = 0; v < n; ++v) root[v] = state[(size_t)v] == 1;
    return rounds;
}

} // namespace sblas

namespace {

using namespace sblas;

struct RefLevel {
    int64_t n;
    const int32_t *rowptr, *colidx, *agg, *aggptr, *members;
    const double *val, *wd;
    std::vector<double> own_b, own_x[2], res;
    const double *b;
    double *x[2];
    const double *table = nullptr; // the Chebyshev smoother's (c1_k, c2_k), the level's own; d is its direction vector
    std::vector<double> d;
};

struct RefOps {
    std::vector<RefLevel> &lv;
    double scale;
    void first(int l, int dst)
    {
        RefLevel &L = lv[(size_t)l];
        for (int64_t i = 0; i < L.n; ++i) L.x[dst][i] = L.wd[i] * L.b[i];
    }
    void sweep(int l, int src, int dst)
    {
        RefLevel &L = lv[(size_t)l];
        for (int64_t i = 0; i < L.n; ++i) {
            const double s = amg_row_sum(L.colidx, L.val, L.rowptr[i], L.rowptr[i + 1], L.x[src]);
            const double d = L.b[i] - s, t = L.wd[i] * d;
            L.x[dst][i] = L.x[src][i] + t;
        }
    }
    void poly_first(int l, int dst)
    {
        RefLevel &L = lv[(size_t)l];
        for (int64_t i = 0; i < L.n; ++i) {
            const double t = L.wd[i] * L.b[i];
            L.d[(size_t)i] = L.table[1] * t;
            L.x[dst][i] = L.d[(size_t)i];
        }
    }
    void poly_guess(int l, int src, int dst) { poly(l, 0, src, dst); }
    void poly_step(int l, int k, int src, int dst) { poly(l, k, src, dst); }
    void poly(int l, int k, int src, int dst)
    {
        RefLevel &L = lv[(size_t)l];
        for (int64_t i = 0; i < L.n; ++i) {
            const double s = amg_row_sum(L.colidx, L.val, L.rowptr[i], L.rowptr[i + 1], L.x[src]);
            const double res = L.b[i] - s, t = L.wd[i] * res;
            double dn = L.table[2 * k + 1] * t;
            if (k > 0) {
                const double kept = L.table[2 * k] * L.d[(size_t)i];
                dn = kept + dn;
            }
            L.d[(size_t)i] = dn;
            L.x[dst][i] = L.x[src][i] + dn;
        }
    }
    void residual(int l, int src)
    {
        RefLevel &L = lv[(size_t)l];
        for (int64_t i = 0; i < L.n; ++i) L.res[(size_t)i] = L.b[i] - amg_row_sum(L.colidx, L.val, L.rowptr[i], L.rowptr[i + 1], L.x[src]);
    }
    void restrict_to(int l)
    {
        RefLevel &L = lv[(size_t)l], &Cs = lv[(size_t)l + 1];
        for (int64_t a = 0; a < Cs.n; ++a) {
            double s = 0.0;
            for (int64_t k = L.aggptr[a]; k < L.aggptr[a + 1]; ++k) s = s + L.res[(size_t)L.members[k]];
            Cs.own_b[(size_t)a] = s;
        }
    }
    void prolong(int l, int dst)
    {
        RefLevel &L = lv[(size_t)l], &Cs = lv[(size_t)l + 1];
        const double *e = Cs.x[AMG_RESULT_BUFFER];
        for (int64_t i = 0; i < L.n; ++i) {
            const double t = scale * e[L.agg[i]];
            L.x[dst][i] = L.x[dst][i] + t;
        }
    }
};

// the rectangular row product of the smoothed plan's transfers: row_sum over every row of M
void transfer_rows(int mode, int64_t rows, const int32_t *rowptr, const int32_t *colidx, const double *val, double scale, const double *in,
                   double *out)
{
    for (int64_t i = 0; i < rows; ++i) {
        const double s = amg_row_sum(colidx, val, rowptr[i], rowptr[i + 1], in);
        if (mode == AMG_RESTRICT) {
            out[i] = s;
        } else {
            const double t = scale * s;
            out[i] = out[i] + t;
        }
    }
}

// the walk's transfers with general P and R; everything else is RefOps'
struct RefOpsSa : RefOps {
    const int32_t *const *p_rowptr, *const *p_colidx, *const *r_rowptr, *const *r_colidx;
    const double *const *p_val, *const *r_val;
    void restrict_to(int l)
    {
        RefLevel &L = lv[(size_t)l], &Cs = lv[(size_t)l + 1];
        transfer_rows(AMG_RESTRICT, Cs.n, r_rowptr[l], r_colidx[l], r_val[l], 0.0, L.res.data(), Cs.own_b.data());
    }
    void prolong(int l, int dst)
    {
        RefLevel &L = lv[(size_t)l], &Cs = lv[(size_t)l + 1];
        transfer_rows(AMG_PROLONG, L.n, p_rowptr[l], p_colidx[l], p_val[l], scale, Cs.x[AMG_RESULT_BUFFER], L.x[dst]);
    }
};

// the vectors of the reference levels: level 0 reads the caller's r and ends in the caller's z
void ref_levels(std::vector<RefLevel> &lv, const int64_t *n, const int32_t *const *rowptr, const int32_t *const *colidx, const double *const *val,
                const double *const *wd, const double *r, double *z, const double *const *table = nullptr)
{
    const int levels = (int)lv.size();
    for (int l = 0; l < levels; ++l) {
        RefLevel &L = lv[(size_t)l];
        const bool last = l + 1 == levels;
        L.n = n[l], L.rowptr = rowptr[l], L.colidx = colidx[l], L.val = val[l], L.wd = wd[l];
        L.agg = L.aggptr = L.members = nullptr;
        if (table) L.table = table[l], L.d.assign((size_t)L.n, 0.0);
        L.own_x[0].assign((size_t)L.n, 0.0), L.res.assign(last ? 0 : (size_t)L.n, 0.0);
        L.x[0] = L.own_x[0].data();
        if (l == 0) {
            L.b = r, L.x[1] = z;
        } else {
            L.own_b.assign((size_t)L.n, 0.0), L.own_x[1].assign((size_t)L.n, 0.0);
            L.b = L.own_b.data(), L.x[1] = L.own_x[1].data();
        }
    }
}

} // namespace

extern "C" {

int sblas_amg_keep_level(int64_t n, int64_t n_next, double min_reduction)
{
    if (n < 0 || n_next < 0 || !amg_min_reduction_ok(min_reduction)) return -1;
    return amg_keep_level(n, n_next, min_reduction) ? 1 : 0;
}

int sblas_amg_prolongator_ref(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, const int32_t *agg, int64_t n_agg,
                              double prolong_omega, int32_t *p_rowptr, int32_t *p_colidx, double *p_val, int64_t *p_nnz, int64_t *bad_row)
{
    if (bad_row) *bad_row = -1;
    if (p_nnz) *p_nnz = 0;
    if (n < 0 || n > INT_MAX || n_agg < 0 || n_agg > INT_MAX || !rowptr || !p_rowptr || !p_nnz) return SBLAS_E_INVALID;
    if (!amg_prolong_omega_ok(prolong_omega)) return SBLAS_E_INVALID;
    if (n > 0 && (!agg || (rowptr[n] > 0 && (!colidx || !val)))) return SBLAS_E_INVALID;
    for (int64_t i = 0; i < n; ++i)
        if (agg[i] < 0 || agg[i] >= n_agg) return SBLAS_E_INVALID;
    std::vector<std::pair<int32_t, double>> row; // (agg[col(e)], t_e) in stored order
    int64_t count = 0;
    p_rowptr[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        int64_t dp = -1;
        for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
            if (colidx[e] < 0 || colidx[e] >= n) {
                if (bad_row) *bad_row = i;
                return SBLAS_E_INVALID;
            }
            if (colidx[e] == i && dp < 0) dp = e;
        }
        if (dp < 0) {
            if (bad_row) *bad_row = i;
            return SBLAS_E_INVALID;
        }
        const double q = prolong_omega / val[dp];
        row.clear();
        for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
            const double prod = q * val[e];
            row.emplace_back(agg[colidx[e]], e == dp ? 1.0 - prod : -prod);
        }
        // the COO plan's order: by column, equal columns in input order, each run added left to right
        std::stable_sort(row.begin(), row.end(), [](const std::pair<int32_t, double> &a, const std::pair<int32_t, double> &b) { return a.first < b.first; });
        for (size_t k = 0; k < row.size();) {
            double v = row[k].second;
            size_t j = k + 1;
            for (; j < row.size() && row[j].first == row[k].first; ++j) v = v + row[j].second;
            if (p_colidx) p_colidx[count] = row[k].first;
            if (p_val) p_val[count] = v;
            ++count, k = j;
        }
        if (count > INT_MAX) return SBLAS_E_INVALID;
        p_rowptr[i + 1] = (int32_t)count;
    }
    *p_nnz = count;
    return SBLAS_OK;
}

int sblas_amg_transfer_ref(int mode, int64_t rows, const int32_t *rowptr, const int32_t *colidx, const double *val, double scale,
                           const double *in, double *out)
{
    if ((mode != AMG_RESTRICT && mode != AMG_PROLONG) || rows < 0 || rows > INT_MAX || !rowptr) return SBLAS_E_INVALID;
    if (rows > 0 && (!out || out == in || (rowptr[rows] > 0 && (!colidx || !val || !in)))) return SBLAS_E_INVALID;
    transfer_rows(mode, rows, rowptr, colidx, val, scale, in, out);
    return SBLAS_OK;
}

int sblas_amg_cycle_sa_ref(int levels, const int64_t *n, const int32_t *const *rowptr, const int32_t *const *colidx, const double *const *val,
                           const double *const *wd, const int32_t *const *p_rowptr, const int32_t *const *p_colidx, const double *const *p_val,
                           const int32_t *const *r_rowptr, const int32_t *const *r_colidx, const double *const *r_val, int nu,
                           int coarse_sweeps, double coarse_scale, const double *r, double *z)
{
    return sblas_amg_cycle_cheb_sa_ref(levels, n, rowptr, colidx, val, wd, nullptr, p_rowptr, p_colidx, p_val, r_rowptr, r_colidx, r_val, nu, 0,
                                       coarse_sweeps, coarse_scale, r, z);
}

int sblas_amg_cycle_cheb_sa_ref(int levels, const int64_t *n, const int32_t *const *rowptr, const int32_t *const *colidx, const double *const *val,
                                const double *const *wd, const double *const *table, const int32_t *const *p_rowptr,
                                const int32_t *const *p_colidx, const double *const *p_val, const int32_t *const *r_rowptr,
                                const int32_t *const *r_colidx, const double *const *r_val, int nu, int degree, int coarse_sweeps,
                                double coarse_scale, const double *r, double *z)
{
    if (!amg_cycle_args_ok(levels, nu, coarse_sweeps)) return SBLAS_E_INVALID;
    if (degree != 0 && (!amg_cheb_args_ok(degree, coarse_sweeps) || (levels > 0 && !table))) return SBLAS_E_INVALID;
    if (levels == 0) return SBLAS_OK;
    for (int l = 0; degree != 0 && l < levels; ++l)
        if (!table[l]) return SBLAS_E_INVALID;
    if (!n || !rowptr || !colidx || !val || !wd) return SBLAS_E_INVALID;
    if (levels > 1 && (!p_rowptr || !p_colidx || !p_val || !r_rowptr || !r_colidx || !r_val)) return SBLAS_E_INVALID;
    for (int l = 0; l < levels; ++l) {
        if (n[l] < 0 || n[l] > INT_MAX || !rowptr[l]) return SBLAS_E_INVALID;
        if (n[l] > 0 && (!wd[l] || (rowptr[l][n[l]] > 0 && (!colidx[l] || !val[l])))) return SBLAS_E_INVALID;
        if (l + 1 < levels) {
            if (!p_rowptr[l] || !r_rowptr[l]) return SBLAS_E_INVALID;
            if (p_rowptr[l][n[l]] > 0 && (!p_colidx[l] || !p_val[l])) return SBLAS_E_INVALID;
            if (n[l + 1] >= 0 && r_rowptr[l][n[l + 1]] > 0 && (!r_colidx[l] || !r_val[l])) return SBLAS_E_INVALID;
        }
    }
    if (n[0] > 0 && (!r || !z || r == z)) return SBLAS_E_INVALID;
    std::vector<RefLevel> lv((size_t)levels);
    ref_levels(lv, n, rowptr, colidx, val, wd, r, z, degree != 0 ? table : nullptr);
    RefOpsSa ops{{lv, coarse_scale}, p_rowptr, p_colidx, r_rowptr, r_colidx, p_val, r_val};
    amg_cycle(levels, nu, coarse_sweeps, ops, 0, degree);
    return SBLAS_OK;
}

int sblas_amg_limits(int64_t out[8])
{
    if (!out) return SBLAS_E_INVALID;
    out[0] = AMG_G4_MAX, out[1] = AMG_G16_MAX, out[2] = AMG_THREADS, out[3] = AMG_COARSE_MAX, out[4] = AMG_MAX_LEVELS;
    out[5] = AMG_NU, out[6] = AMG_COARSE_SWEEPS, out[7] = AMG_LEVEL_CAP;
    return SBLAS_OK;
}

// the block cycle's sizes (amg_multi.h)
int sblas_amg_multi_limits(int64_t out[4])
{
    if (!out) return SBLAS_E_INVALID;
    out[0] = SBLAS_AMG_MULTI_MAX_RHS, out[1] = TILE, out[2] = AMG_THREADS, out[3] = 0;
    return SBLAS_OK;
}

int sblas_amg_multi_grid(int64_t units, int nrhs, int64_t out[4])
{
    if (!out || units < 0 || !amg_multi_width_ok(nrhs)) return SBLAS_E_INVALID;
    out[0] = unit_blocks(units, AMG_UNITS_PER_BLOCK), out[1] = tiles(nrhs), out[2] = out[0] * out[1];
    out[3] = nrhs - (int)(out[1] - 1) * TILE;
    return SBLAS_OK;
}

int sblas_amg_aggregate(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, double theta, uint32_t seed,
                        uint32_t level, int32_t *agg, int32_t *aggptr, int32_t *members, int64_t *n_agg, int64_t *bad_row)
{
    if (bad_row) *bad_row = -1;
    if (n_agg) *n_agg = 0;
    if (n < 0 || n > INT_MAX || !rowptr || !aggptr || !n_agg) return SBLAS_E_INVALID;
    if (!amg_theta_ok(theta) || (theta > 0.0 && !val)) return SBLAS_E_INVALID;
    if (n > 0 && (!agg || !members)) return SBLAS_E_INVALID;
    const int rc = sblas_ilu0_check(n, rowptr, colidx, nullptr, bad_row);
    if (rc != SBLAS_OK) return rc;
    std::vector<int32_t> ptr;
    *n_agg = amg_aggregate(n, rowptr, colidx, val, theta, seed, level, agg, ptr, members);
    for (size_t a = 0; a < ptr.size(); ++a) aggptr[a] = ptr[a];
    return SBLAS_OK;
}

int sblas_amg_roots_rounds_ref(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, double theta, uint32_t seed,
                               uint32_t level, unsigned char *root_out, int64_t *rounds, int64_t *bad_row)
{
    if (bad_row) *bad_row = -1;
    if (rounds) *rounds = 0;
    if (n < 0 || n > INT_MAX || !rowptr || !rounds) return SBLAS_E_INVALID;
    if (!amg_theta_ok(theta) || (theta > 0.0 && !val)) return SBLAS_E_INVALID;
    if (n > 0 && !root_out) return SBLAS_E_INVALID;
    const int rc = sblas_ilu0_check(n, rowptr, colidx, nullptr, bad_row);
    if (rc != SBLAS_OK) return rc;
    const int64_t r = amg_roots_rounds(n, rowptr, colidx, val, theta, seed, level, root_out);
    if (r < 0) return SBLAS_E_INTERNAL;
    *rounds = r;
    return SBLAS_OK;
}

int64_t sblas_amg_launches(int levels, int nu, int coarse_sweeps)
{
    if (!amg_cycle_args_ok(levels, nu, coarse_sweeps)) return -1;
    AmgCount c;
    amg_cycle(levels, nu, coarse_sweeps, c);
    return c.n;
}

int sblas_amg_wd_ref(int64_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, int smoother, double omega, double *wd,
                     int64_t *bad_row)
{
    if (bad_row) *bad_row = -1;
    if (n < 0 || n > INT_MAX || !rowptr || (smoother != SBLAS_AMG_JACOBI && smoother != SBLAS_AMG_L1)) return SBLAS_E_INVALID;
    if (n > 0 && (!colidx || !val || !wd)) return SBLAS_E_INVALID;
    for (int64_t i = 0; i < n; ++i) {
        double d = 0.0, l1 = 0.0;
        bool found = false;
        for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
            if (colidx[e] == i) d = val[e], found = true;
            l1 = l1 + fabs(val[e]);
        }
        if (!found) {
            if (bad_row) *bad_row = i;
            return SBLAS_E_INVALID;
        }
        wd[i] = omega / (smoother == SBLAS_AMG_L1 ? l1 : d);
        if (!(isfinite(d) && d > 0.0) && bad_row && *bad_row < 0) *bad_row = i; // reported, not refused: as the device flags it
    }
    return SBLAS_OK;
}

int64_t sblas_amg_launches_cheb(int levels, int nu, int coarse_sweeps, int degree)
{
    if (!amg_cycle_args_ok(levels, nu, coarse_sweeps) || !amg_cheb_args_ok(degree, coarse_sweeps)) return -1;
    AmgCount c;
    amg_cycle(levels, nu, coarse_sweeps, c, 0, degree);
    return c.n;
}

int sblas_amg_cycle_ref(int levels, const int64_t *n, const int32_t *const *rowptr, const int32_t *const *colidx, const double *const *val,
                        const double *const *wd, const int32_t *const *agg, const int32_t *const *aggptr, const int32_t *const *members,
                        int nu, int coarse_sweeps, double coarse_scale, const double *r, double *z)
{
    return sblas_amg_cycle_cheb_ref(levels, n, rowptr, colidx, val, wd, nullptr, agg, aggptr, members, nu, 0, coarse_sweeps, coarse_scale, r, z);
}

int sblas_amg_cycle_cheb_ref(int levels, const int64_t *n, const int32_t *const *rowptr, const int32_t *const *colidx, const double *const *val,
                             const double *const *wd, const double *const *table, const int32_t *const *agg, const int32_t *const *aggptr,
                             const int32_t *const *members, int nu, int degree, int coarse_sweeps, double coarse_scale, const double *r,
                             double *z)
{
    if (!amg_cycle_args_ok(levels, nu, coarse_sweeps)) return SBLAS_E_INVALID;
    if (degree != 0 && (!amg_cheb_args_ok(degree, coarse_sweeps) || (levels > 0 && !table))) return SBLAS_E_INVALID;
    if (levels == 0) return SBLAS_OK;
    for (int l = 0; degree != 0 && l < levels; ++l)
        if (!table[l]) return SBLAS_E_INVALID;
    if (!n || !rowptr || !colidx || !val || !wd) return SBLAS_E_INVALID;
    if (levels > 1 && (!agg || !aggptr || !members)) return SBLAS_E_INVALID;
    for (int l = 0; l < levels; ++l) {
        if (n[l] < 0 || n[l] > INT_MAX || !rowptr[l]) return SBLAS_E_INVALID;
        if (n[l] > 0 && (!wd[l] || (rowptr[l][n[l]] > 0 && (!colidx[l] || !val[l])))) return SBLAS_E_INVALID;
        if (l + 1 < levels && n[l] > 0 && (!agg[l] || !aggptr[l] || !members[l])) return SBLAS_E_INVALID;
    }
    if (n[0] > 0 && (!r || !z || r == z)) return SBLAS_E_INVALID;
    std::vector<RefLevel> lv((size_t)levels);
    for (int l = 0; l < levels; ++l) {
        RefLevel &L = lv[(size_t)l];
        const bool last = l + 1 == levels;
        L.n = n[l], L.rowptr = rowptr[l], L.colidx = colidx[l], L.val = val[l], L.wd = wd[l];
        L.agg = last ? nullptr : agg[l], L.aggptr = last ? nullptr : aggptr[l], L.members = last ? nullptr : members[l];
        if (degree != 0) L.table = table[l], L.d.assign((size_t)L.n, 0.0);
        L.own_x[0].assign((size_t)L.n, 0.0), L.res.assign(last ? 0 : (size_t)L.n, 0.0);
        L.x[0] = L.own_x[0].data();
        if (l == 0) {
            L.b = r, L.x[1] = z;
        } else {
            L.own_b.assign((size_t)L.n, 0.0), L.own_x[1].assign((size_t)L.n, 0.0);
            L.b = L.own_b.data(), L.x[1] = L.own_x[1].data();
        }
    }
    RefOps ops{lv, coarse_scale};
    amg_cycle(levels, nu, coarse_sweeps, ops, 0, degree);
    return SBLAS_OK;
}

} // extern "C"
