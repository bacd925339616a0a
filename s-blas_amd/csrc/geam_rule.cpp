// geam_rule.cpp -- the host side of the GEAM plan (sblas_hip_geam_plan_create, geam.hip): the limit on nnz(C) and the
// contract of include/sblas_hip_geam.h as a scalar loop, structure, values and both maps.  No GPU call in this file, so
// it is testable on a CPU box (tools/geam_rule_check.cpp builds it alone under a host sanitizer).
#include <limits.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../../include/sblas_hip.h"

// alpha * a and t1 + t2 are separate roundings
#pragma clang fp contract(off)

namespace {

// rowptr starts at 0 and never steps down; every column of its nnz entries is inside [0, cols)
bool structure_ok(int64_t rows, int64_t cols, const int32_t *rowptr, const int32_t *colidx)
{
    if (!rowptr || rowptr[0] != 0) return false;
    for (int64_t i = 0; i < rows; ++i)
        if (rowptr[i + 1] < rowptr[i]) return false;
    const int64_t nnz = rowptr[rows];
    if (nnz > 0 && !colidx) return false;
    for (int64_t e = 0; e < nnz; ++e)
        if (colidx[e] < 0 || (int64_t)colidx[e] >= cols) return false;
    return true;
}

struct Term {
    int32_t col;
    int64_t pos; // >= 0: entry pos of A; < 0: entry -pos - 1 of B
};

} // namespace

extern "C" {

// nnz(C) must stay an int32 index
int sblas_geam_check_nnz(int64_t nnz_c)
{
    return nnz_c >= 0 && nnz_c <= INT_MAX ? SBLAS_OK : SBLAS_E_INVALID;
}

int sblas_geam_ref(int64_t rows, int64_t cols, const int32_t *rowptr_a, const int32_t *colidx_a, const double *val_a,
                   const int32_t *rowptr_b, const int32_t *colidx_b, const double *val_b, double alpha, double beta,
                   int32_t *rowptr_c, int32_t *colidx_c, double *val_c, int32_t *dest_a, int32_t *dest_b, int64_t *nnz_c)
{
    if (rows < 0 || cols < 0 || rows > INT_MAX || cols > INT_MAX || !rowptr_c || !nnz_c) return SBLAS_E_INVALID;
    if (!structure_ok(rows, cols, rowptr_a, colidx_a) || !structure_ok(rows, cols, rowptr_b, colidx_b)) return SBLAS_E_INVALID;
    if (val_c && ((rowptr_a[rows] > 0 && !val_a) || (rowptr_b[rows] > 0 && !val_b))) return SBLAS_E_INVALID;
    if (sblas_geam_check_nnz((int64_t)rowptr_a[rows] + rowptr_b[rows]) != SBLAS_OK) { // the sum may still fit: count first
        int64_t count = 0;
        std::vector<int32_t> cols_of_row;
        for (int64_t i = 0; i < rows; ++i) {
            cols_of_row.assign(colidx_a + rowptr_a[i], colidx_a + rowptr_a[i + 1]);
            cols_of_row.insert(cols_of_row.end(), colidx_b + rowptr_b[i], colidx_b + rowptr_b[i + 1]);
            std::sort(cols_of_row.begin(), cols_of_row.end());
            count += std::unique(cols_of_row.begin(), cols_of_row.end()) - cols_of_row.begin();
        }
        if (sblas_geam_check_nnz(count) != SBLAS_OK) return SBLAS_E_INVALID;
    }
    std::vector<Term> terms;
    int64_t out = 0;
    rowptr_c[0] = 0;
    for (int64_t i = 0; i < rows; ++i) {
        terms.clear();
        for (int64_t e = rowptr_a[i]; e < rowptr_a[i + 1]; ++e) terms.push_back(Term{colidx_a[e], e});
        for (int64_t e = rowptr_b[i]; e < rowptr_b[i + 1]; ++e) terms.push_back(Term{colidx_b[e], -e - 1});
        // by column, equal columns in the order of the list: A's in stored order, then B's
        std::stable_sort(terms.begin(), terms.end(), [](const Term &x, const Term &y) { return x.col < y.col; });
        for (size_t t = 0; t < terms.size(); ++t) {
            const bool head = t == 0 || terms[t].col != terms[t - 1].col;
            if (head) {
                if (colidx_c) colidx_c[out] = terms[t].col;
                ++out;
            }
            const int64_t entry = out - 1, pos = terms[t].pos;
            if (pos >= 0 && dest_a) dest_a[pos] = (int32_t)entry;
            if (pos < 0 && dest_b) dest_b[-pos - 1] = (int32_t)entry;
            if (val_c) {
                const double term = pos >= 0 ? alpha * val_a[pos] : beta * val_b[-pos - 1];
                val_c[entry] = head ? term : val_c[entry] + term; // a run of one is copied
            }
        }
        rowptr_c[i + 1] = (int32_t)out;
    }
    *nnz_c = out;
    return SBLAS_OK;
}

} // extern "C"
