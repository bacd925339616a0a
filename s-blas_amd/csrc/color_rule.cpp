// color_rule.cpp -- the host rule of the multicolour ordering (sblas_hip_color_plan_create, color.hip): the structure
// check, the colour of every vertex and the number of rounds of the synchronous parallel form.  Pure functions of host
// arrays; no GPU call in this file, so it is testable on a CPU box.
//
// u is a neighbour of v when u != v and the pattern stores (v, u) or (u, v); duplicates and the diagonal do not matter.
// The vertices are visited in descending h(v) = fmix32(v + 0x9E3779B9 * (seed + 1)), and color[v] is the smallest
// c >= 0 that no already-coloured neighbour holds.  A vertex's colour depends only on its neighbours of higher h, so the
// parallel form -- every uncoloured vertex without an uncoloured neighbour of higher h takes its first fit -- gives the
// same colours under every schedule.  round(v) = 1 + the greatest round among the neighbours of higher h (1 without
// any) is the round in which v is coloured when a round sees only the colours of the rounds before it.
#include <limits.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../../include/sblas_hip.h"
#include "color.h"

namespace sblas {

int color_check_transpose(int64_t n, const int32_t *rowptr, const int32_t *colidx, std::vector<int32_t> &tptr,
                          std::vector<int32_t> &tidx, int64_t *bad_row)
{
    if (bad_row) *bad_row = -1;
    // the row pointers first: nothing indexes colidx before they are known to be sound
    if (rowptr[0] != 0) {
        if (bad_row) *bad_row = 0;
        return SBLAS_E_INVALID;
    }
    for (int64_t i = 0; i < n; ++i)
        if (rowptr[i + 1] < rowptr[i]) {
            if (bad_row) *bad_row = i;
            return SBLAS_E_INVALID;
        }
    const int64_t nnz = rowptr[n];
    if (nnz > 0 && !colidx) return SBLAS_E_INVALID;
    // then every row, in row order: columns in range
    tptr.assign((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
            const int64_t c = colidx[e];
            if (c < 0 || c >= n) {
                if (bad_row) *bad_row = i;
                return SBLAS_E_INVALID;
            }
            ++tptr[(size_t)c + 1];
        }
    for (int64_t c = 0; c < n; ++c) tptr[(size_t)c + 1] += tptr[(size_t)c];
    tidx.resize((size_t)nnz);
    std::vector<int32_t> at(tptr.begin(), tptr.end() - 1);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) tidx[(size_t)at[colidx[e]]++] = (int32_t)i;
    return SBLAS_OK;
}

} // namespace sblas

extern "C" {

int sblas_hip_color_limits(int64_t out[4])
{
    if (!out) return SBLAS_E_INVALID;
    out[0] = sblas::COLOR_G4_MAX, out[1] = sblas::COLOR_G16_MAX, out[2] = sblas::COLOR_WINDOW, out[3] = sblas::COLOR_THREADS;
    return SBLAS_OK;
}

int sblas_csr_color(int64_t n, const int32_t *rowptr, const int32_t *colidx, uint32_t seed, int32_t *color_out, int64_t *n_colors,
                    int64_t *sync_rounds, int64_t *bad_row)
{
    if (bad_row) *bad_row = -1;
    if (n_colors) *n_colors = 0;
    if (sync_rounds) *sync_rounds = 0;
    if (n < 0 || n > INT_MAX || !rowptr || !n_colors) return SBLAS_E_INVALID;
    if (n > 0 && !color_out) return SBLAS_E_INVALID;
    std::vector<int32_t> tptr, tidx;
    const int rc = sblas::color_check_transpose(n, rowptr, colidx, tptr, tidx, bad_row);
    if (rc != SBLAS_OK) return rc;

    const uint32_t salt = sblas::color_salt(seed);
    std::vector<uint64_t> order((size_t)n); // (h, v), descending: h alone decides, no two are equal
    for (int64_t v = 0; v < n; ++v) order[(size_t)v] = ((uint64_t)sblas::color_priority((uint32_t)v, salt) << 32) | (uint64_t)v;
    std::sort(order.begin(), order.end(), [](uint64_t a, uint64_t b) { return a > b; });

    for (int64_t v = 0; v < n; ++v) color_out[v] = -1;
    std::vector<int32_t> round((size_t)n, 0), taken((size_t)n + 1, -1); // taken[c] == v: a neighbour of v holds c
    int64_t top = -1, rounds = 0;
    for (int64_t k = 0; k < n; ++k) {
        const int32_t v = (int32_t)(order[(size_t)k] & 0xffffffffu);
        int32_t r = 0;
        auto meet = [&](int32_t u) { // every coloured neighbour has a higher h: it was visited before
            if (u == v || color_out[u] < 0) return;
            taken[(size_t)color_out[u]] = v;
            r = round[(size_t)u] > r ? round[(size_t)u] : r;
        };
        for (int64_t e = rowptr[v]; e < rowptr[v + 1]; ++e) meet(colidx[e]);
        for (int64_t e = tptr[(size_t)v]; e < tptr[(size_t)v + 1]; ++e) meet(tidx[(size_t)e]);
        int32_t c = 0;
        while (taken[(size_t)c] == v) ++c; // at most the number of distinct neighbours, which is below n
        color_out[v] = c;
        round[(size_t)v] = r + 1;
        top = c > top ? c : top;
        rounds = r + 1 > rounds ? r + 1 : rounds;
    }
    *n_colors = top + 1;
    if (sync_rounds) *sync_rounds = rounds;
    return SBLAS_OK;
}

} // extern "C"
