// spmm_split.cpp -- the host half of a split SpMM plan (sblas_hip_spmm_plan_create_split): which rows are cut into
// pieces that run on workgroups of their own.  A pure function of the row pointers and the plan's panel verdicts; no
// GPU call in this file, so it is testable on a CPU box.
//
// The direct kernels compute a row inside one workgroup (a row per wave, or the sixteen waves together from DPP_LONG
// entries on).  A row of 10^5-10^6 entries then keeps one CU busy while the rest of the chip waits at the end of the
// launch.  Rows of split_min+ entries in panels the plan gives to the direct kernels are cut here into pieces of at most
// `piece` consecutive entries; the pieces are summed by as many workgroups and folded in piece order (kernels.hip,
// spmm_split_piece_kernel / spmm_split_fold_kernel).  Rows in panels of the LDS-tiled, lane-group or matrix-core kernels,
// and rows the row-merging kernel takes, are never split: the caller masks those panels out.  The records are those of
// every split row (split_rows, kernels.h); this file keeps SpMM's choice of rows.
#include <stdint.h>
#include "../../include/sblas_hip.h"
#include "kernels.h"

extern "C" int64_t sblas_spmm_split_classify(const int32_t *rowptr, int64_t rows, int64_t nnz, int64_t split_min,
                                             int64_t piece, const uint8_t *direct_mask, int64_t panel_rows, int32_t *out,
                                             int64_t max_out)
{
    if (rows < 0 || nnz < 0 || (rows > 0 && !rowptr) || (out && max_out < 0) || (direct_mask && panel_rows <= 0)) return -1;
    if (split_min <= 0) split_min = SBLAS_SPMM_SPLIT_MIN;
    if (piece <= 0) piece = SBLAS_SPMM_SPLIT_PIECE;
    if (rows > 0 && (rowptr[0] < 0 || rowptr[rows] > nnz)) return -1;
    auto split = [&](int64_t r, int64_t len) { return len >= split_min && (!direct_mask || direct_mask[r / panel_rows]); };
    return sblas::split_rows(rowptr, rows, piece, split, out, max_out);
}
