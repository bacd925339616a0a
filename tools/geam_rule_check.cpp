// geam_rule_check.cpp -- a stand-alone program over the GEAM plan's host side (s-blas_amd/csrc/geam_rule.cpp; no GPU, no
// HIP runtime), made to be built with a host sanitizer:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/geam_rule_check.cpp \
//       s-blas_amd/csrc/geam_rule.cpp -o /tmp/geam_rule_check && /tmp/geam_rule_check
// It adds small pairs (rows = 0, a single column, empty operands, identical, disjoint and nested patterns, unsorted rows,
// duplicates on either side and on both) out of arrays of exactly the sizes the contract names -- first a counting call
// with every optional output NULL, then a call into arrays of exactly nnz(C) entries -- so that a read or write past
// either end is the sanitizer's to find, and holds structure, value bits and both maps against a second, naive
// restatement: an ordered map per row, filled with A's terms and then B's.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <map>
#include <vector>
#include "../include/sblas_hip.h"

#pragma clang fp contract(off)

struct Csr {
    std::vector<int32_t> rowptr{0}, colidx;
    std::vector<double> val;
    void row(const std::vector<std::pair<int32_t, double>> &r)
    {
        for (const auto &cv : r) colidx.push_back(cv.first), val.push_back(cv.second);
        rowptr.push_back((int32_t)colidx.size());
    }
};

static int failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond), ++failures; \
    } while (0)

static bool same_bits(double x, double y)
{
    if (x != x || y != y) return (x != x) == (y != y); // which NaN is the adder's choice
    return memcmp(&x, &y, 8) == 0;
}

static void check_pair(const char *name, int64_t rows, int64_t cols, const Csr &a, const Csr &b, double alpha, double beta)
{
    const size_t na = a.colidx.size(), nb = b.colidx.size();
    // the naive restatement
    std::vector<int32_t> rp{0}, ci, da(na), db(nb);
    std::vector<double> v;
    for (int64_t i = 0; i < rows; ++i) {
        std::map<int32_t, std::vector<int64_t>> terms; // column -> the terms that land on it, A's (pos) then B's (-pos - 1)
        for (int32_t e = a.rowptr[i]; e < a.rowptr[i + 1]; ++e) terms[a.colidx[e]].push_back(e);
        for (int32_t e = b.rowptr[i]; e < b.rowptr[i + 1]; ++e) terms[b.colidx[e]].push_back(-(int64_t)e - 1);
        for (const auto &kv : terms) {
            double acc = 0.0;
            for (size_t t = 0; t < kv.second.size(); ++t) {
                const int64_t p = kv.second[t];
                const double term = p >= 0 ? alpha * a.val[p] : beta * b.val[-p - 1];
                acc = t == 0 ? term : acc + term;
                (p >= 0 ? da[p] : db[-p - 1]) = (int32_t)ci.size();
            }
            ci.push_back(kv.first), v.push_back(acc);
        }
        rp.push_back((int32_t)ci.size());
    }
    // count, then fill arrays of exactly that size
    std::vector<int32_t> rowptr_c((size_t)rows + 1, -7);
    int64_t nnz_c = -7;
    int rc = sblas_geam_ref(rows, cols, a.rowptr.data(), na ? a.colidx.data() : nullptr, nullptr, b.rowptr.data(), nb ? b.colidx.data() : nullptr,
                            nullptr, alpha, beta, rowptr_c.data(), nullptr, nullptr, nullptr, nullptr, &nnz_c);
    EXPECT(rc == SBLAS_OK && nnz_c == (int64_t)ci.size());
    if (rc != SBLAS_OK || nnz_c != (int64_t)ci.size()) {
        printf("  in %s\n", name);
        return;
    }
    std::vector<int32_t> colidx_c((size_t)nnz_c), dest_a(na), dest_b(nb);
    std::vector<double> val_c((size_t)nnz_c);
    rc = sblas_geam_ref(rows, cols, a.rowptr.data(), na ? a.colidx.data() : nullptr, na ? a.val.data() : nullptr, b.rowptr.data(),
                        nb ? b.colidx.data() : nullptr, nb ? b.val.data() : nullptr, alpha, beta, rowptr_c.data(),
                        nnz_c ? colidx_c.data() : nullptr, nnz_c ? val_c.data() : nullptr, na ? dest_a.data() : nullptr,
                        nb ? dest_b.data() : nullptr, &nnz_c);
    EXPECT(rc == SBLAS_OK);
    EXPECT(rowptr_c == rp && colidx_c == ci && dest_a == da && dest_b == db);
    bool bits = true;
    for (size_t e = 0; e < v.size(); ++e) bits = bits && same_bits(val_c[e], v[e]);
    EXPECT(bits);
    if (failures) printf("  in %s (alpha %g, beta %g)\n", name, alpha, beta);
}

int main()
{
    const double inf = HUGE_VAL, scalars[5] = {1.0, -1.0, 0.0, 0.5, 3e200};
    std::vector<std::pair<const char *, std::pair<Csr, Csr>>> cases;
    std::vector<std::pair<int64_t, int64_t>> shapes;
    auto add = [&](const char *name, int64_t cols, const Csr &a, const Csr &b) {
        cases.push_back({name, {a, b}});
        shapes.push_back({(int64_t)a.rowptr.size() - 1, cols});
    };
    Csr none, e3, a, b, c, d, u, dup, dup2, one, one2;
    for (int i = 0; i < 3; ++i) e3.row({});
    a.row({{0, 1.5}, {2, -0.0}, {5, 1e16}}), a.row({}), a.row({{1, inf}, {3, 5e-324}});
    b.row({{0, 0.25}, {2, 0.0}, {5, -1e16}}), b.row({{4, 2.0}}), b.row({{1, -inf}, {3, 5e-324}});
    c.row({{1, 1.0}, {3, 2.0}}), c.row({{0, 3.0}}), c.row({});
    d.row({{2, 1.0}}), d.row({{0, -3.0}, {5, 1.0}}), d.row({{5, 7.0}});
    u.row({{5, 1.0}, {0, 2.0}, {3, 3.0}}), u.row({{4, 1.0}, {1, 1.0}}), u.row({{2, 1.0}});
    dup.row({{3, 1e16}, {1, 2.0}, {3, 1.0}}), dup.row({}), dup.row({{0, 0.1}, {0, 0.2}, {0, 0.3}});
    dup2.row({{4, 1.0}, {3, -1e16}, {3, 5.0}}), dup2.row({{2, 1.0}, {2, 0x1p-60}}), dup2.row({{0, 0.7}});
    one.row({{0, 1.0 / 3.0}}), one.row({}), one2.row({{0, 1.0 / 3.0}}), one2.row({{0, 2.0}});
    add("rows0", 4, none, none), add("both_empty", 6, e3, e3), add("a_empty", 6, e3, b), add("b_empty", 6, a, e3);
    add("identical", 6, a, b), add("disjoint", 6, c, d), add("subset", 6, c, u), add("unsorted", 6, u, a);
    add("dup_a", 6, dup, b), add("dup_b", 6, a, dup), add("dup_both", 6, dup, dup2), add("cols1", 1, one, one2);
    for (size_t k = 0; k < cases.size(); ++k)
        for (double alpha : scalars)
            for (double beta : scalars) check_pair(cases[k].first, shapes[k].first, shapes[k].second, cases[k].second.first, cases[k].second.second, alpha, beta);
    // no contraction: 3 * fl(1/3) rounds to 1, so the sum with -3 * fl(1/3) is +0.0
    {
        int32_t rpc[3];
        int32_t cic[2];
        double vc[2];
        int64_t n = 0;
        EXPECT(sblas_geam_ref(2, 1, one.rowptr.data(), one.colidx.data(), one.val.data(), one2.rowptr.data(), one2.colidx.data(), one2.val.data(),
                              3.0, -3.0, rpc, cic, vc, nullptr, nullptr, &n) == SBLAS_OK);
        EXPECT(n == 2 && vc[0] == 0.0 && !signbit(vc[0]) && vc[1] == -6.0);
    }
    // refusals: nothing is written through a bad structure
    {
        std::vector<int32_t> rpc(4, -7);
        int64_t n = -7;
        Csr bad = a;
        bad.rowptr[0] = 1;
        EXPECT(sblas_geam_ref(3, 6, bad.rowptr.data(), bad.colidx.data(), nullptr, b.rowptr.data(), b.colidx.data(), nullptr, 1, 1, rpc.data(),
                              nullptr, nullptr, nullptr, nullptr, &n) == SBLAS_E_INVALID);
        bad = a, bad.rowptr[1] = 5, bad.rowptr[2] = 4;
        EXPECT(sblas_geam_ref(3, 6, a.rowptr.data(), a.colidx.data(), nullptr, bad.rowptr.data(), bad.colidx.data(), nullptr, 1, 1, rpc.data(),
                              nullptr, nullptr, nullptr, nullptr, &n) == SBLAS_E_INVALID);
        bad = a, bad.colidx[4] = 6;
        EXPECT(sblas_geam_ref(3, 6, bad.rowptr.data(), bad.colidx.data(), nullptr, b.rowptr.data(), b.colidx.data(), nullptr, 1, 1, rpc.data(),
                              nullptr, nullptr, nullptr, nullptr, &n) == SBLAS_E_INVALID);
        EXPECT(sblas_geam_ref(3, 6, a.rowptr.data(), a.colidx.data(), nullptr, b.rowptr.data(), b.colidx.data(), nullptr, 1, 1, nullptr, nullptr,
                              nullptr, nullptr, nullptr, &n) == SBLAS_E_INVALID);
        EXPECT(n == -7 && rpc == std::vector<int32_t>(4, -7));
    }
    EXPECT(sblas_geam_check_nnz(0) == SBLAS_OK && sblas_geam_check_nnz(((int64_t)1 << 31) - 1) == SBLAS_OK);
    EXPECT(sblas_geam_check_nnz((int64_t)1 << 31) == SBLAS_E_INVALID && sblas_geam_check_nnz(-1) == SBLAS_E_INVALID);
    if (failures) {
        printf("geam_rule_check: %d failure(s)\n", failures);
        return 1;
    }
    printf("geam_rule_check: %zu pairs x 25 scalar pairs, the contraction pair, the refusals and the limit: ok\n", cases.size());
    return 0;
}
