// mspgemm_rule_check.cpp -- a stand-alone program over the masked SpGEMM plan's host side
// (s-blas_amd/csrc/mspgemm_rule.cpp; no GPU, no HIP runtime), made to be built with a host sanitizer:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/mspgemm_rule_check.cpp \
//       s-blas_amd/csrc/mspgemm_rule.cpp -o /tmp/mspgemm_rule_check && /tmp/mspgemm_rule_check
// It multiplies small triples (every dimension 0 in turn, empty operands, a 1 x 1, unsorted rows, duplicates in the mask,
// in X and in Y, special values) out of arrays of exactly the sizes the contract names, so that a read or write past
// either end is the sanitizer's to find, and holds the value bits against a second, naive restatement: per mask entry
// the list of matched pairs, gathered first and summed afterwards.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <utility>
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
    int64_t rows() const { return (int64_t)rowptr.size() - 1; }
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

template <typename T> static const T *ptr(const std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }

static int call(int64_t m, int64_t n, int64_t k, const Csr &mask, const Csr &x, const Csr &y, std::vector<double> &out)
{
    return sblas_mspgemm_ref(m, n, k, mask.rowptr.data(), ptr(mask.colidx), x.rowptr.data(), ptr(x.colidx), ptr(x.val), y.rowptr.data(),
                             ptr(y.colidx), ptr(y.val), out.empty() ? nullptr : out.data());
}

static void check_triple(const char *name, int64_t k, const Csr &mask, const Csr &x, const Csr &y)
{
    const int64_t m = mask.rows(), n = y.rows();
    std::vector<double> want;
    for (int64_t i = 0; i < m; ++i) {
        for (int32_t t = mask.rowptr[i]; t < mask.rowptr[i + 1]; ++t) {
            const int32_t j = mask.colidx[t];
            std::vector<double> products; // (e, g) with e the major index, both in stored order
            for (int32_t e = x.rowptr[i]; e < x.rowptr[i + 1]; ++e)
                for (int32_t g = y.rowptr[j]; g < y.rowptr[j + 1]; ++g)
                    if (x.colidx[e] == y.colidx[g]) products.push_back(x.val[e] * y.val[g]);
            double acc = 0.0;
            for (size_t q = 0; q < products.size(); ++q) acc = q == 0 ? products[q] : acc + products[q];
            want.push_back(acc);
        }
    }
    std::vector<double> out(mask.colidx.size(), -7.0);
    const int rc = call(m, n, k, mask, x, y, out);
    EXPECT(rc == SBLAS_OK);
    bool bits = rc == SBLAS_OK;
    for (size_t t = 0; t < want.size() && bits; ++t) bits = same_bits(out[t], want[t]);
    EXPECT(bits);
    if (rc != SBLAS_OK || !bits) printf("  in %s\n", name);
}

int main()
{
    const double inf = HUGE_VAL;
    Csr none, e3, e4, m34, x3, y4, xu, yu, xd, yd, md, m11, x11, y11, xs, ys;
    for (int i = 0; i < 3; ++i) e3.row({});
    for (int i = 0; i < 4; ++i) e4.row({});
    m34.row({{0, 0}, {2, 0}, {3, 0}}), m34.row({}), m34.row({{1, 0}, {3, 0}});
    x3.row({{0, 1.5}, {2, -0.0}, {4, 1e16}}), x3.row({{1, 2.0}}), x3.row({{1, 1.0 / 3.0}, {3, 5e-324}});
    y4.row({{0, 0.25}, {2, 5.0}}), y4.row({{1, 3.0}, {3, 1.0}}), y4.row({}), y4.row({{1, -3.0}, {4, -1.0}});
    xu.row({{4, 1.0}, {0, 2.0}, {2, 3.0}}), xu.row({}), xu.row({{3, 1.0}, {1, -1.0}});
    yu.row({{2, 1.0}, {0, 1.0}}), yu.row({{3, 2.0}, {1, 2.0}, {4, 0.5}}), yu.row({{4, 1.0}}), yu.row({{1, 1.0}, {3, 1.0}, {0, 7.0}});
    xd.row({{3, 1e16}, {1, 1.0}, {3, -1e16}}), xd.row({{0, 0.1}, {0, 0.2}, {0, 0.3}}), xd.row({{2, 1.0}});
    yd.row({{1, 1.0}, {3, 1.0}}), yd.row({{0, 1.0}, {0, 1e-3}}), yd.row({{2, 1e16}, {0, 9.0}, {2, 1.0}, {2, -1e16}}), yd.row({{3, 2.0}, {3, 2.0}});
    md.row({{0, 0}, {0, 0}, {3, 0}}), md.row({{1, 0}, {1, 0}, {2, 0}}), md.row({{2, 0}, {2, 0}});
    m11.row({{0, 0}}), x11.row({{0, 1.0 / 3.0}}), y11.row({{0, 3.0}});
    xs.row({{0, inf}, {2, 2.0}, {4, 0.0}}), xs.row({{1, -0.0}}), xs.row({{0, inf}});
    ys.row({{2, 3.0}, {1, inf}}), ys.row({{4, inf}, {3, NAN}}), ys.row({{0, 1.0}, {0, -1.0}}), ys.row({{1, 4.0}});
    struct Case {
        const char *name;
        int64_t k;
        const Csr *mask, *x, *y;
    } cases[] = {{"all0", 0, &none, &none, &none}, {"m0", 5, &none, &none, &y4},    {"n0", 5, &e3, &x3, &none},     {"k0", 0, &m34, &e3, &e4},
                 {"mask_empty", 5, &e3, &x3, &y4}, {"x_empty", 5, &m34, &e3, &y4},  {"y_empty", 5, &m34, &x3, &e4}, {"sorted", 5, &m34, &x3, &y4},
                 {"unsorted", 5, &m34, &xu, &yu},  {"dup_x", 5, &m34, &xd, &y4},    {"dup_y", 5, &m34, &x3, &yd},   {"dup_all", 5, &md, &xd, &yd},
                 {"one_by_one", 1, &m11, &x11, &y11}, {"special", 5, &m34, &xs, &ys}};
    for (const Case &c : cases) check_triple(c.name, c.k, *c.mask, *c.x, *c.y);
    // the named values: a single product is copied, no pair is +0.0, the order is X's, an unmatched Inf stays out
    {
        std::vector<double> out(5);
        EXPECT(call(3, 4, 5, m34, x3, y4, out) == SBLAS_OK);
        EXPECT(out[0] == 0.375 && out[1] == 0.0 && !signbit(out[1]) && out[2] == -1e16); // row 0 x Y rows 0, 2 (empty), 3
        EXPECT(out[3] == 1.0 && out[4] == -1.0);                                         // fl(fl(1/3) * 3); fl(1/3) * -3
        Csr mz;
        mz.row({{0, 0}}), mz.row({}), mz.row({});
        Csr yz;
        yz.row({{2, 5.0}}), yz.row({}), yz.row({}), yz.row({});
        std::vector<double> one(1);
        EXPECT(call(3, 4, 5, mz, x3, yz, one) == SBLAS_OK && one[0] == 0.0 && signbit(one[0])); // -0.0 * 5 alone
        std::vector<double> d(8);
        EXPECT(call(3, 4, 5, md, xd, yd, d) == SBLAS_OK && d[0] == 0.0 && d[1] == 0.0); // (1e16 + 1) + -1e16, the duplicate alike
        std::vector<double> s(5);
        EXPECT(call(3, 4, 5, m34, xs, ys, s) == SBLAS_OK && s[0] == 6.0 && s[1] != s[1] && s[2] == 0.0); // Inf - Inf on Y's row 2
    }
    // refusals: nothing is written through a bad structure
    {
        std::vector<double> out(5, -7.0);
        const std::vector<double> untouched(5, -7.0);
        Csr bad = m34;
        bad.rowptr[0] = 1;
        EXPECT(call(3, 4, 5, bad, x3, y4, out) == SBLAS_E_INVALID);
        bad = x3, bad.rowptr[1] = 5, bad.rowptr[2] = 4;
        EXPECT(call(3, 4, 5, m34, bad, y4, out) == SBLAS_E_INVALID);
        bad = m34, bad.colidx[2] = 4; // a mask column = n
        EXPECT(call(3, 4, 5, bad, x3, y4, out) == SBLAS_E_INVALID);
        bad = x3, bad.colidx[2] = 5; // an X column = k
        EXPECT(call(3, 4, 5, m34, bad, y4, out) == SBLAS_E_INVALID);
        bad = y4, bad.colidx[0] = -1;
        EXPECT(call(3, 4, 5, m34, x3, bad, out) == SBLAS_E_INVALID);
        EXPECT(call(-1, 4, 5, m34, x3, y4, out) == SBLAS_E_INVALID);
        std::vector<double> missing;
        EXPECT(call(3, 4, 5, m34, x3, y4, missing) == SBLAS_E_INVALID);
        EXPECT(sblas_mspgemm_ref(3, 4, 5, nullptr, nullptr, x3.rowptr.data(), x3.colidx.data(), x3.val.data(), y4.rowptr.data(), y4.colidx.data(),
                                 y4.val.data(), out.data()) == SBLAS_E_INVALID);
        EXPECT(out == untouched);
    }
    int64_t lim[4] = {-1, -1, -1, -1};
    EXPECT(sblas_mspgemm_limits(lim) == SBLAS_OK && lim[0] >= 64 && lim[1] >= 64 && lim[1] % 64 == 0 && lim[2] == 0 && lim[3] == 0);
    EXPECT(sblas_mspgemm_limits(nullptr) == SBLAS_E_INVALID);
    if (failures) {
        printf("mspgemm_rule_check: %d failure(s)\n", failures);
        return 1;
    }
    printf("mspgemm_rule_check: %zu triples, the named values, the refusals and the limits: ok\n", sizeof(cases) / sizeof(cases[0]));
    return 0;
}
