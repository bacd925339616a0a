// sddmm_narrow_rule_check.cpp -- a stand-alone program over the narrow SDDMM's host side
// (s-blas_amd/csrc/sddmm_narrow_rule.cpp; no GPU, no HIP runtime), made to be built with a host sanitizer:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/sddmm_narrow_rule_check.cpp \
//       s-blas_amd/csrc/sddmm_narrow_rule.cpp -o /tmp/sddmm_narrow_rule_check && /tmp/sddmm_narrow_rule_check
// It runs small patterns (rows = 0, nnz = 0, empty rows, duplicates, unsorted columns) at every k, part and a few
// alpha / beta out of arrays of exactly the sizes the contract names -- X and Y end with their last row's k-th element,
// whatever the leading dimension -- so that a read or write past either end is the sanitizer's to find, fills the rows
// that only entries outside the part name with NaN, and holds every value against a second, naive restatement.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../include/sblas_hip.h"

#pragma clang fp contract(off)

static int failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond), ++failures; \
    } while (0)

static bool same_bits(double x, double y) { return memcmp(&x, &y, 8) == 0; }

static bool inside(int part, int r, int c)
{
    switch (part) {
    case SBLAS_PART_LOWER: return c <= r;
    case SBLAS_PART_UPPER: return c >= r;
    case SBLAS_PART_STRICT_LOWER: return c < r;
    case SBLAS_PART_STRICT_UPPER: return c > r;
    default: return true;
    }
}

// the naive restatement: the padded sum written out per width
static double naive_dot(const double *x, const double *y, int k)
{
    double px[8] = {0, 0, 0, 0, 0, 0, 0, 0}, py[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < k; ++j) px[j] = x[j], py[j] = y[j];
    if (k <= 2) return fma(px[1], py[1], fma(px[0], py[0], 0.0));
    if (k <= 4) return fma(px[3], py[3], fma(px[2], py[2], fma(px[1], py[1], fma(px[0], py[0], 0.0))));
    const double s0 = fma(px[5], py[5], fma(px[4], py[4], fma(px[1], py[1], fma(px[0], py[0], 0.0))));
    const double s1 = fma(px[7], py[7], fma(px[6], py[6], fma(px[3], py[3], fma(px[2], py[2], 0.0))));
    return s0 + s1;
}

static void check_case(const char *name, int rows, int cols, const std::vector<int32_t> &rowptr, const std::vector<int32_t> &colidx)
{
    const int64_t nnz = (int64_t)colidx.size();
    const double scalars[3][2] = {{1.0, 0.0}, {-1.0, 1.0}, {0.5, -2.0}};
    for (int k = 1; k <= 8; ++k)
        for (int pad = 0; pad <= 3; pad += 3)
            for (int part = SBLAS_PART_ALL; part <= SBLAS_PART_STRICT_UPPER; ++part)
                for (const auto &ab : scalars) {
                    const int64_t ld = k + pad;
                    // exactly (r - 1) * ld + k doubles: the padding behind the last row does not exist
                    std::vector<double> X(rows ? (size_t)((rows - 1) * ld + k) : 0), Y(cols ? (size_t)((cols - 1) * ld + k) : 0);
                    for (size_t i = 0; i < X.size(); ++i) X[i] = (double)((i * 7 + 3) % 11) - 5.0 + 1.0 / (double)(i + 3);
                    for (size_t i = 0; i < Y.size(); ++i) Y[i] = (double)((i * 5 + 1) % 13) - 6.0 + 1.0 / (double)(i + 7);
                    std::vector<char> x_read((size_t)rows, 0), y_read((size_t)cols, 0);
                    for (int r = 0; r < rows; ++r)
                        for (int e = rowptr[r]; e < rowptr[r + 1]; ++e)
                            if (inside(part, r, colidx[e])) x_read[r] = 1, y_read[colidx[e]] = 1;
                    for (int r = 0; r < rows; ++r)
                        if (!x_read[r])
                            for (int j = 0; j < k; ++j) X[r * ld + j] = NAN;
                    for (int c = 0; c < cols; ++c)
                        if (!y_read[c])
                            for (int j = 0; j < k; ++j) Y[c * ld + j] = INFINITY;
                    std::vector<double> out((size_t)nnz), old((size_t)nnz);
                    for (int64_t e = 0; e < nnz; ++e) old[e] = out[e] = ab[1] == 0.0 ? NAN : 0.25 * (double)(e + 1); // beta == 0 never reads out
                    const int rc = sblas_sddmm_narrow_ref(-1, nullptr, rows, cols, nnz, rowptr.data(), nnz ? colidx.data() : nullptr,
                                                          X.empty() ? nullptr : X.data(), ld, Y.empty() ? nullptr : Y.data(), ld, k, ab[0],
                                                          ab[1], part, nnz ? out.data() : nullptr);
                    EXPECT(rc == SBLAS_OK);
                    bool bits = true;
                    for (int r = 0; r < rows; ++r)
                        for (int e = rowptr[r]; e < rowptr[r + 1]; ++e) {
                            double want;
                            if (!inside(part, r, colidx[e])) want = ab[1] == 0.0 ? 0.0 : ab[1] * old[e];
                            else {
                                const double sres = ab[0] * naive_dot(&X[r * ld], &Y[colidx[e] * ld], k);
                                want = ab[1] == 0.0 ? sres : fma(ab[1], old[e], sres);
                            }
                            bits = bits && same_bits(out[e], want) && isfinite(out[e]);
                        }
                    EXPECT(bits);
                    if (failures) {
                        printf("  in %s (k %d, ld %d, part %d, alpha %g, beta %g)\n", name, k, (int)ld, part, ab[0], ab[1]);
                        return;
                    }
                }
}

int main()
{
    check_case("rows0", 0, 0, {0}, {});
    check_case("nnz0", 3, 4, {0, 0, 0, 0}, {});
    check_case("one", 3, 3, {0, 0, 1, 1}, {0});
    check_case("square", 5, 5, {0, 3, 3, 5, 9, 10}, {4, 0, 2, 2, 1, 3, 0, 3, 4, 0});   // empty row, unsorted, a duplicate
    check_case("wide", 3, 7, {0, 2, 6, 7}, {6, 0, 5, 1, 1, 3, 2});
    check_case("tall", 6, 2, {0, 1, 2, 2, 4, 5, 6}, {1, 0, 0, 1, 1, 0});
    // the padded step: a product that underflows makes the sum -0, and fma(+0, +0, -0), which k = 1 pads with, makes it +0
    {
        const int32_t rp[2] = {0, 1}, ci[1] = {0};
        const double x = -1e-200, y = 1e-200;
        double out = NAN;
        EXPECT(sblas_sddmm_narrow_ref(-1, nullptr, 1, 1, 1, rp, ci, &x, 1, &y, 1, 1, 1.0, 0.0, SBLAS_PART_ALL, &out) == SBLAS_OK);
        EXPECT(out == 0.0 && !signbit(out));
    }
    // refusals: out is not written
    {
        const int32_t rp[3] = {0, 1, 2}, ci[2] = {0, 1}, bad_rp[3] = {0, 2, 1}, bad_ci[2] = {0, 2};
        const double X[4] = {1, 2, 3, 4};
        double out[2] = {-7.0, -7.0};
        int64_t lim[4] = {0, 0, 0, 0};
#define REF(rows, cols, nnz, rp_, ci_, ldx, ldy, k, part) \
    sblas_sddmm_narrow_ref(-1, nullptr, rows, cols, nnz, rp_, ci_, X, ldx, X, ldy, k, 1.0, 0.0, part, out)
        EXPECT(REF(2, 2, 2, rp, ci, 2, 2, 2, SBLAS_PART_ALL) == SBLAS_OK && out[0] == 5.0 && out[1] == 25.0);
        out[0] = out[1] = -7.0;
        EXPECT(REF(2, 2, 2, rp, ci, 2, 2, 0, SBLAS_PART_ALL) == SBLAS_E_INVALID);
        EXPECT(REF(2, 2, 2, rp, ci, 2, 2, 9, SBLAS_PART_ALL) == SBLAS_E_INVALID);
        EXPECT(REF(2, 2, 2, rp, ci, 1, 2, 2, SBLAS_PART_ALL) == SBLAS_E_INVALID);
        EXPECT(REF(2, 2, 2, rp, ci, 2, 1, 2, SBLAS_PART_ALL) == SBLAS_E_INVALID);
        EXPECT(REF(2, 2, 2, rp, ci, 2, 2, 2, 5) == SBLAS_E_INVALID);
        EXPECT(REF(2, 2, 2, rp, ci, 2, 2, 2, -1) == SBLAS_E_INVALID);
        EXPECT(REF(2, 2, 2, bad_rp, ci, 2, 2, 2, SBLAS_PART_ALL) == SBLAS_E_INVALID);
        EXPECT(REF(2, 2, 2, rp, bad_ci, 2, 2, 2, SBLAS_PART_ALL) == SBLAS_E_INVALID);
        EXPECT(REF(2, 2, 1, rp, ci, 2, 2, 2, SBLAS_PART_ALL) == SBLAS_E_INVALID);
        EXPECT(REF(2, 0, 2, rp, ci, 2, 2, 2, SBLAS_PART_ALL) == SBLAS_E_INVALID);
        EXPECT(REF((int64_t)1 << 31, 2, 2, rp, ci, 2, 2, 2, SBLAS_PART_ALL) == SBLAS_E_INVALID);
        EXPECT(REF(2, (int64_t)1 << 31, 2, rp, ci, 2, 2, 2, SBLAS_PART_ALL) == SBLAS_E_INVALID);
        EXPECT(REF(2, 2, (int64_t)1 << 31, rp, ci, 2, 2, 2, SBLAS_PART_ALL) == SBLAS_E_INVALID);
        EXPECT(REF(2, 2, 2, nullptr, ci, 2, 2, 2, SBLAS_PART_ALL) == SBLAS_E_INVALID);
#undef REF
        EXPECT(out[0] == -7.0 && out[1] == -7.0);
        EXPECT(sblas_sddmm_narrow_limits(lim) == SBLAS_OK && lim[0] == 8 && lim[1] == lim[2] * lim[3] && lim[2] % 64 == 0);
        EXPECT(sblas_sddmm_narrow_limits(nullptr) == SBLAS_E_INVALID);
    }
    if (failures) {
        printf("sddmm_narrow_rule_check: %d failure(s)\n", failures);
        return 1;
    }
    printf("sddmm_narrow_rule_check: 6 patterns x 8 widths x 2 leading dimensions x 5 parts x 3 scalar pairs, the padded step, "
           "the refusals and the limits: ok\n");
    return 0;
}
