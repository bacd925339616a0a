// fsai_rule_check.cpp -- a stand-alone program over the FSAI plan's host rule (s-blas_amd/csrc/fsai_rule.cpp with ILU(0)'s
// structure check from ilu0_plan.cpp; no GPU, no HIP runtime), made to be built with a host sanitizer:
//   clang++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/fsai_rule_check.cpp \
//       s-blas_amd/csrc/fsai_rule.cpp s-blas_amd/csrc/ilu0_plan.cpp -o /tmp/fsai_rule_check && /tmp/fsai_rule_check
// (g++ takes the same line).  It runs the pattern function (A's lower part, a caller's pattern, every max_row) and the
// reference on small matrices -- n = 0 and 1, a diagonal, a tridiagonal, a grid with the pattern of its square, a band, a
// clique above 64, an indefinite 2 x 2 -- out of arrays of exactly the sizes the contract names, so that a read or write
// past either end is the sanitizer's to find, and holds what comes back against what must be true of it: the pattern's
// shape, the unit diagonal of G A G^T on the positive definite cases, the diagonal fallback on a failed row.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <map>
#include <utility>
#include <vector>
#include "../include/sblas_hip.h"

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
    double at(int64_t i, int64_t j) const
    {
        for (int32_t e = rowptr[(size_t)i]; e < rowptr[(size_t)i + 1]; ++e)
            if (colidx[(size_t)e] == j) return val[(size_t)e];
        return 0.0;
    }
};

static Csr band(int n, int half, double diag)
{
    Csr a;
    for (int i = 0; i < n; ++i) {
        std::map<int32_t, double> r;
        for (int j = i - half < 0 ? 0 : i - half; j <= i + half && j < n; ++j) r[j] = i == j ? diag : -1.0 / ((i > j ? i - j : j - i) + 1);
        a.row(r);
    }
    return a;
}

static Csr grid(int side)
{
    Csr a;
    for (int y = 0; y < side; ++y)
        for (int x = 0; x < side; ++x) {
            std::map<int32_t, double> r;
            r[y * side + x] = 4.0;
            if (x > 0) r[y * side + x - 1] = -1.0;
            if (x + 1 < side) r[y * side + x + 1] = -1.0;
            if (y > 0) r[(y - 1) * side + x] = -1.0;
            if (y + 1 < side) r[(y + 1) * side + x] = -1.0;
            a.row(r);
        }
    return a;
}

// the pattern of A^2, whole rows: the pattern function drops what lies above the diagonal
static Csr squared_pattern(const Csr &a)
{
    Csr p;
    for (int64_t i = 0; i < a.n; ++i) {
        std::map<int32_t, double> r;
        for (int32_t e = a.rowptr[(size_t)i]; e < a.rowptr[(size_t)i + 1]; ++e) {
            const int32_t k = a.colidx[(size_t)e];
            for (int32_t f = a.rowptr[(size_t)k]; f < a.rowptr[(size_t)k + 1]; ++f) r[a.colidx[(size_t)f]] = 1.0;
        }
        p.row(r);
    }
    return p;
}

static int bad = 0;
static void expect(bool ok, const char *what, const char *name)
{
    if (!ok) ++bad, fprintf(stderr, "fsai_rule_check: %s: %s\n", name, what);
}

// spd: every dense system is positive definite.  pat: the caller's pattern, or NULL.
static void run(const char *name, const Csr &a, const Csr *pat, int max_row, bool spd)
{
    const int64_t n = a.n;
    const int32_t *rp = a.rowptr.data(), *ci = a.colidx.data();
    const int64_t source = pat ? (int64_t)pat->colidx.size() : (int64_t)a.colidx.size();
    std::vector<int32_t> grp((size_t)n + 1, -1), counted((size_t)n + 1, -1), gci((size_t)source);
    int64_t row = 0;
    const int32_t *prp = pat ? pat->rowptr.data() : nullptr, *pci = pat ? pat->colidx.data() : nullptr;
    expect(sblas_fsai_pattern(n, rp, ci, pat ? source : 0, prp, pci, max_row, counted.data(), nullptr, &row) == SBLAS_OK && row == -1, "the count accepts", name);
    expect(sblas_fsai_pattern(n, rp, ci, pat ? source : 0, prp, pci, max_row, grp.data(), gci.data(), &row) == SBLAS_OK && row == -1, "the pattern accepts", name);
    expect(grp == counted && grp[0] == 0 && grp[(size_t)n] <= source, "the count is the pattern's", name);
    gci.resize((size_t)grp[(size_t)n]); // exactly what was written: the reference reads no more
    for (int64_t i = 0; i < n; ++i) {
        const int32_t beg = grp[(size_t)i], end = grp[(size_t)i + 1];
        expect(end > beg && end - beg <= 64 && (max_row == 0 || end - beg <= max_row), "a row has 1 .. 64 entries, at most max_row", name);
        expect(gci[(size_t)end - 1] == i, "a row ends on its diagonal", name);
        for (int32_t e = beg + 1; e < end; ++e) expect(gci[(size_t)e] > gci[(size_t)e - 1], "a row ascends", name);
    }
    std::vector<double> g(gci.size());
    expect(sblas_fsai_ref(n, rp, ci, a.val.data(), grp.data(), gci.data(), g.data(), &row) == SBLAS_OK, "the reference accepts", name);
    if (!spd) return;
    expect(row == -1, "no row fails on a positive definite matrix", name);
    // (G A G^T)_ii = sum_pq g_p A[J_p][J_q] g_q = 1
    for (int64_t i = 0; i < n; ++i) {
        double s = 0.0;
        for (int32_t p = grp[(size_t)i]; p < grp[(size_t)i + 1]; ++p)
            for (int32_t q = grp[(size_t)i]; q < grp[(size_t)i + 1]; ++q) {
                const int32_t r = gci[(size_t)p], c = gci[(size_t)q];
                s += g[(size_t)p] * (r >= c ? a.at(r, c) : a.at(c, r)) * g[(size_t)q];
            }
        expect(fabs(s - 1.0) <= 1e-12, "the diagonal of G A G^T is 1", name);
        expect(g[(size_t)grp[(size_t)i + 1] - 1] > 0.0, "g_ii > 0", name);
    }
}

int main()
{
    Csr n0, n1, diagonal, clique, indefinite;
    n1.row({{0, 2.0}});
    for (int i = 0; i < 37; ++i) diagonal.row({{i, 1.0 + i % 7}});
    for (int i = 0; i < 70; ++i) {
        std::map<int32_t, double> r;
        for (int j = 0; j < 70; ++j) r[j] = i == j ? 3.0 : -0.01 * (1 + (i + j) % 3);
        clique.row(r);
    }
    indefinite.row({{0, 1.0}, {1, 2.0}});
    indefinite.row({{0, 2.0}, {1, 1.0}});
    const Csr tri = band(300, 1, 2.5), b6 = band(200, 6, 4.0), b20 = band(150, 20, 8.0), g9 = grid(9), g9sq = squared_pattern(g9);
    run("n0", n0, nullptr, 0, true);
    run("n1", n1, nullptr, 0, true);
    run("diagonal37", diagonal, nullptr, 0, true);
    run("tridiagonal300", tri, nullptr, 0, true);
    run("grid9", g9, nullptr, 0, true);
    run("grid9 squared", g9, &g9sq, 0, true);
    run("grid9 squared, max_row 4", g9, &g9sq, 4, true);
    run("band6", b6, nullptr, 0, true);
    for (int k : {0, 1, 2, 8, 21, 64}) run("band20", b20, nullptr, k, true);
    for (int k : {1, 33, 64}) run("clique70", clique, nullptr, k, true);
    run("indefinite2", indefinite, nullptr, 0, false);

    const char *r = "refusals";
    int64_t row = 0;
    std::vector<int32_t> grp(71), gci(70 * 70);
    expect(sblas_fsai_limits(nullptr) != SBLAS_OK, "limits needs out", r);
    expect(sblas_fsai_pattern(clique.n, clique.rowptr.data(), clique.colidx.data(), 0, nullptr, nullptr, 0, grp.data(), gci.data(), &row) == SBLAS_E_INVALID && row == 64,
           "a row above 64 is refused and named", r);
    for (int k : {-1, 65})
        expect(sblas_fsai_pattern(g9.n, g9.rowptr.data(), g9.colidx.data(), 0, nullptr, nullptr, k, grp.data(), gci.data(), &row) != SBLAS_OK, "max_row is checked", r);
    expect(sblas_fsai_pattern(g9.n, g9.rowptr.data(), g9.colidx.data(), 0, nullptr, nullptr, 0, nullptr, gci.data(), &row) != SBLAS_OK, "the pattern needs out_rowptr", r);
    Csr no_diag = g9sq; // row 4's diagonal becomes a second column 5: the row no longer ascends
    for (int32_t e = no_diag.rowptr[4]; e < no_diag.rowptr[5]; ++e)
        if (no_diag.colidx[(size_t)e] == 4) no_diag.colidx[(size_t)e] = 5;
    expect(sblas_fsai_pattern(g9.n, g9.rowptr.data(), g9.colidx.data(), (int64_t)no_diag.colidx.size(), no_diag.rowptr.data(), no_diag.colidx.data(), 0, grp.data(),
                              gci.data(), &row) == SBLAS_E_INVALID && row == 4,
           "a pattern row that does not ascend is named", r);
    Csr strict; // the strictly lower part of the tridiagonal: row 0 is empty, no row holds its diagonal
    for (int i = 0; i < 300; ++i) strict.row(i ? std::map<int32_t, double>{{i - 1, 1.0}} : std::map<int32_t, double>{});
    expect(sblas_fsai_pattern(tri.n, tri.rowptr.data(), tri.colidx.data(), (int64_t)strict.colidx.size(), strict.rowptr.data(), strict.colidx.data(), 0, grp.data(),
                              gci.data(), &row) == SBLAS_E_INVALID && row == 0,
           "a pattern row without its diagonal is named", r);
    Csr unsorted = g9;
    std::swap(unsorted.colidx[(size_t)unsorted.rowptr[7]], unsorted.colidx[(size_t)unsorted.rowptr[7] + 1]);
    expect(sblas_fsai_pattern(unsorted.n, unsorted.rowptr.data(), unsorted.colidx.data(), 0, nullptr, nullptr, 0, grp.data(), gci.data(), &row) == SBLAS_E_INVALID && row == 7,
           "ILU(0)'s check names A's first bad row", r);
    // the indefinite block: row 1 fails and is its diagonal alone
    std::vector<double> g(3);
    expect(sblas_fsai_pattern(2, indefinite.rowptr.data(), indefinite.colidx.data(), 0, nullptr, nullptr, 0, grp.data(), gci.data(), &row) == SBLAS_OK && grp[2] == 3,
           "the 2 x 2 pattern", r);
    expect(sblas_fsai_ref(2, indefinite.rowptr.data(), indefinite.colidx.data(), indefinite.val.data(), grp.data(), gci.data(), g.data(), &row) == SBLAS_OK && row == 1 &&
               g[0] == 1.0 && g[1] == 0.0 && g[2] == 1.0,
           "a failed row is its diagonal alone and is reported", r);
    Csr planted = g9;
    for (double what : {-4.0, 0.0, (double)NAN, (double)INFINITY}) {
        planted.val[(size_t)planted.rowptr[40] + 2] = what; // row 40 of the 9 x 9 grid stores 31, 39, 40, 41, 49
        std::vector<int32_t> prp(82), pci(planted.colidx.size());
        sblas_fsai_pattern(planted.n, planted.rowptr.data(), planted.colidx.data(), 0, nullptr, nullptr, 0, prp.data(), pci.data(), &row);
        std::vector<double> pg((size_t)prp[81]);
        expect(sblas_fsai_ref(planted.n, planted.rowptr.data(), planted.colidx.data(), planted.val.data(), prp.data(), pci.data(), pg.data(), &row) == SBLAS_OK && row == 40,
               "a planted diagonal is reported, not refused", r);
        expect(pg[(size_t)prp[41] - 1] == 1.0 && pg[(size_t)prp[40]] == 0.0, "the fallback of a diagonal that is not > 0 is 1", r);
    }
    expect(sblas_fsai_ref(2, indefinite.rowptr.data(), indefinite.colidx.data(), indefinite.val.data(), grp.data(), gci.data(), nullptr, &row) != SBLAS_OK,
           "the reference needs val_g", r);
    if (bad) return fprintf(stderr, "fsai_rule_check: %d failures\n", bad), 1;
    printf("fsai_rule_check: ok\n");
    return 0;
}
