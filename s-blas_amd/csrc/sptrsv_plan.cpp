// sptrsv_plan.cpp -- the host rule of the triangular-solve plan (sblas_hip_sptrsv_plan_create, sptrsv.hip): the structure
// checks, the level of every row, and the cut of the levels into launches.  Pure functions of host arrays; no GPU call
// in this file, so it is testable on a CPU box.
//
// The selected entries of row i are its stored entries with column < i (SBLAS_FILL_LOWER) or > i (SBLAS_FILL_UPPER);
// entries in the other triangle are ignored, and so are stored diagonals under SBLAS_DIAG_UNIT.  level(i) = 0 when row i
// selects nothing, else 1 + the greatest level among the rows its selected entries name: the rows of one level do not
// depend on each other.
#include <limits.h>
#include <stdint.h>
#include "../../include/sblas_hip.h"
#include "sptrsv.h"
#include "sptrsm_tile.h"

extern "C" {

int sblas_hip_sptrsv_limits(int64_t out[4])
{
    if (!out) return SBLAS_E_INVALID;
    out[0] = sblas::SPTRSV_CHAIN_ROWS, out[1] = sblas::SPTRSV_CHAIN_THREADS, out[2] = sblas::SPTRSV_G4_MAX, out[3] = sblas::SPTRSV_G16_MAX;
    return SBLAS_OK;
}

// the tiled SpSM's sizes (sptrsm_tile.h)
int sblas_sptrsm_tile_limits(int64_t out[4])
{
    if (!out) return SBLAS_E_INVALID;
    out[0] = sblas::TILE, out[1] = sblas::SPTRSM_WIDE_THREADS, out[2] = sblas::SPTRSV_CHAIN_THREADS, out[3] = sblas::SPTRSM_MAX_GRID;
    return SBLAS_OK;
}

int sblas_sptrsm_tile_grid(int64_t units, int64_t nrhs, int64_t out[4])
{
    if (!out || units < 0 || nrhs < 1) return SBLAS_E_INVALID;
    const int64_t blocks = sblas::unit_blocks(units, sblas::SPTRSM_UNITS_PER_BLOCK), grid = sblas::tile_grid(blocks, nrhs);
    if (grid < 0) return SBLAS_E_INVALID;
    out[0] = blocks, out[1] = sblas::tiles(nrhs), out[2] = grid;
    out[3] = nrhs - (out[1] - 1) * sblas::TILE;
    return SBLAS_OK;
}

int sblas_sptrsv_levels(int64_t n, const int32_t *rowptr, const int32_t *colidx, int fill, int diag, int32_t *level_out,
                        int64_t *n_levels, int64_t *bad_row)
{
    if (bad_row) *bad_row = -1;
    if (n_levels) *n_levels = 0;
    if (n < 0 || n > INT_MAX || !rowptr || !n_levels) return SBLAS_E_INVALID;
    if (fill != SBLAS_FILL_LOWER && fill != SBLAS_FILL_UPPER) return SBLAS_E_INVALID;
    if (diag != SBLAS_DIAG_NON_UNIT && diag != SBLAS_DIAG_UNIT) return SBLAS_E_INVALID;
    if (n > 0 && !level_out) return SBLAS_E_INVALID;
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
    if (n > 0 && rowptr[n] > 0 && !colidx) return SBLAS_E_INVALID;
    // then every row, in row order: columns in range, and one stored diagonal unless the diagonal is implied
    for (int64_t i = 0; i < n; ++i) {
        int64_t on_diag = 0;
        for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
            const int64_t c = colidx[e];
            if (c < 0 || c >= n) {
                if (bad_row) *bad_row = i;
                return SBLAS_E_INVALID;
            }
            on_diag += (c == i);
        }
        if (diag == SBLAS_DIAG_NON_UNIT && on_diag != 1) {
            if (bad_row) *bad_row = i;
            return SBLAS_E_INVALID;
        }
    }
    // a row's level needs the levels of the rows it names: ascending for a lower triangle, descending for an upper
    const bool lower = fill == SBLAS_FILL_LOWER;
    int64_t top = -1;
    for (int64_t k = 0; k < n; ++k) {
        const int64_t i = lower ? k : n - 1 - k;
        int32_t lv = 0;
        for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
            const int64_t c = colidx[e];
            if (lower ? c < i : c > i) lv = level_out[c] + 1 > lv ? level_out[c] + 1 : lv;
        }
        level_out[i] = lv;
        top = lv > top ? lv : top;
    }
    *n_levels = top + 1;
    return SBLAS_OK;
}

int sblas_sptrsv_schedule(int64_t n_levels, const int64_t *widths, int flags, int64_t chain_rows, uint8_t *kind_out,
                          int64_t *launch_first_out, int64_t *n_launches)
{
    if (n_levels < 0 || chain_rows < 0 || !n_launches || !launch_first_out) return SBLAS_E_INVALID;
    if (flags != SBLAS_SPTRSV_AUTO && flags != SBLAS_SPTRSV_PER_LEVEL && flags != SBLAS_SPTRSV_CHAIN_ONLY) return SBLAS_E_INVALID;
    if (n_levels > 0 && (!widths || !kind_out)) return SBLAS_E_INVALID;
    const int64_t narrow = chain_rows > 0 ? chain_rows : sblas::SPTRSV_CHAIN_ROWS;
    int64_t launches = 0;
    bool chain_open = false; // the last launch is a chain that the next narrow level joins
    for (int64_t l = 0; l < n_levels; ++l) {
        if (widths[l] < 0) return SBLAS_E_INVALID;
        const bool chain = flags == SBLAS_SPTRSV_CHAIN_ONLY || (flags == SBLAS_SPTRSV_AUTO && widths[l] <= narrow);
        if (chain && chain_open) continue;
        kind_out[launches] = chain ? SBLAS_SPTRSV_LAUNCH_CHAIN : SBLAS_SPTRSV_LAUNCH_WIDE;
        launch_first_out[launches++] = l;
        chain_open = chain;
    }
    launch_first_out[launches] = n_levels;
    *n_launches = launches;
    return SBLAS_OK;
}

} // extern "C"
