// spgemm_plan.cpp -- the host rule of the SpGEMM plan (sblas_hip_spgemm_plan_create, spgemm.hip): which path takes each
// row of C, how the general rows are cut into chunks, how many lanes a row-path row gets, and the limits both sides
// agree on.  Pure functions of the per-row product counts and column spans the plan's device pass produced; no GPU call
// in this file, so it is testable on a CPU box.
//
// A row with no product has nothing to do on either path (SBLAS_SPGEMM_PATH_EMPTY; its C row is empty).  Every other
// row takes the row path when B's rows are strictly ascending, its column span fits the LDS bitmap (SPGEMM_S_MAX) and
// SBLAS_SPGEMM_GENERAL is not set; otherwise the general path.  The general rows, in row order, are cut greedily into
// chunks of consecutive general rows whose products add up to at most the cap; a row above the cap is a chunk of its
// own.
#include <limits.h>
#include <stdint.h>
#include "../../include/sblas_hip.h"
#include "spgemm.h"

extern "C" {

int sblas_hip_spgemm_limits(int64_t out[4])
{
    if (!out) return SBLAS_E_INVALID;
    out[0] = sblas::SPGEMM_S_MAX, out[1] = sblas::SPGEMM_ACC_CAP, out[2] = sblas::SPGEMM_CHUNK_CAP, out[3] = 0;
    return SBLAS_OK;
}

int sblas_hip_spgemm_classify(int64_t m, const int64_t *products, const int64_t *span, int b_ascending, int flags,
                              int64_t chunk_cap, uint8_t *path, int64_t *chunk_first, int64_t *n_chunks)
{
    if (m < 0 || chunk_cap < 0 || !n_chunks || !chunk_first) return SBLAS_E_INVALID;
    if (flags != SBLAS_SPGEMM_AUTO && flags != SBLAS_SPGEMM_GENERAL) return SBLAS_E_INVALID;
    if (m > 0 && (!products || !span || !path)) return SBLAS_E_INVALID;
    const int64_t cap = chunk_cap > 0 ? chunk_cap : sblas::SPGEMM_CHUNK_CAP;
    const bool row_ok = b_ascending && flags == SBLAS_SPGEMM_AUTO;
    int64_t general = 0, chunks = 0, in_chunk = 0; // general rows so far; products of the open chunk (0: none open)
    for (int64_t i = 0; i < m; ++i) {
        if (products[i] < 0 || span[i] < 0) return SBLAS_E_INVALID;
        if (products[i] == 0) {
            path[i] = SBLAS_SPGEMM_PATH_EMPTY;
        } else if (row_ok && span[i] <= sblas::SPGEMM_S_MAX) {
            path[i] = SBLAS_SPGEMM_PATH_ROW;
        } else {
            path[i] = SBLAS_SPGEMM_PATH_GENERAL;
            // in_chunk <= cap and products[i] <= cap on the right-hand side's reach, so the comparison cannot overflow
            if (in_chunk == 0 || products[i] > cap - in_chunk) {
                chunk_first[chunks++] = general;
                in_chunk = 0;
            }
            in_chunk = products[i] > cap ? cap : in_chunk + products[i]; // a row above the cap closes its chunk
            ++general;
        }
    }
    chunk_first[chunks] = general;
    *n_chunks = chunks;
    return SBLAS_OK;
}

// lanes of the row path for a row of `a_len` stored A entries: the narrow form while the named B rows are short on
// average and the span fits a narrow group's share of the bitmap
int sblas_hip_spgemm_group_width(int64_t products, int64_t a_len, int64_t span)
{
    if (a_len > 0 && span <= sblas::SPGEMM_NARROW_S_MAX && products <= sblas::SPGEMM_NARROW_MEAN * a_len) return sblas::SPGEMM_NARROW;
    return 64;
}

// nnz(C) must stay an int32 index
int sblas_hip_spgemm_check_nnz(int64_t nnz_c)
{
    return nnz_c >= 0 && nnz_c <= INT_MAX ? SBLAS_OK : SBLAS_E_INVALID;
}

} // extern "C"
