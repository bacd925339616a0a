// spmv_plan.cpp -- the host half of the SpMV plan (sblas_hip_spmv_plan_*): the row-length classifier that cuts a
// matrix into work items.  A pure function of the row pointers; no GPU call in this file, so it is testable on a CPU box.
//
// The unplanned launcher (launch_spmv, spmv_kernels.hip) picks ONE kernel for the whole matrix from nnz / rows.  Here
// the rows are taken in tiles of 256 (the stream kernel's block; every other kernel's block -- 64, 16 and 8 rows --
// divides it) and each tile is classified by the average length of its rows, with the launcher's own thresholds
// (2.5 / 64 / 96 nonzeros per row, the slice-count table of the LDS-window kernel, the run count of the stream kernel).
// A tile whose kernel family is the one the launcher picks for the whole matrix takes exactly the launcher's
// instantiation, so a matrix whose tiles all agree is computed by the same kernel, block for block, as the unplanned
// call.  A tile of another family takes the instantiation its own rows ask for.  A row longer than `split_min` becomes an
// item of its own and is cut into pieces of `piece` nonzeros that run on as many workgroups.
#include <stdint.h>
#include "../../include/sblas_hip.h"

namespace {

constexpr int64_t TILE = 256;
enum { FAM_LPR, FAM_STREAM, FAM_SEG, FAM_LDS };

// the launcher's automatic choice for an average row length (launch_spmv / launch_stream, spmv_kernels.hip)
int stream_kind(double avg)
{
    const double per_block = avg * 256.0;
    const int runs4 = (int)((per_block + 4095.0) / 4096.0), runs6 = (int)((per_block + 6143.0) / 6144.0);
    return runs4 <= runs6 ? SBLAS_SPMV_ITEM_STREAM4096 : SBLAS_SPMV_ITEM_STREAM6144;
}
int lds_kind(double avg)
{
    if (avg <= 115.0) return SBLAS_SPMV_ITEM_LDS_S2;
    if (avg <= 180.0) return SBLAS_SPMV_ITEM_LDS_S3;
    if (avg <= 230.0) return SBLAS_SPMV_ITEM_LDS_S4;
    return SBLAS_SPMV_ITEM_LDS_S7;
}
int family_of(double avg)
{
    if (avg > 96.0) return FAM_LDS;
    if (avg > 64.0) return FAM_SEG;
    if (avg > 2.5) return FAM_STREAM;
    return FAM_LPR;
}
int kind_in(int fam, double avg)
{
    switch (fam) {
    case FAM_LDS: return lds_kind(avg);
    case FAM_SEG: return SBLAS_SPMV_ITEM_SEG;
    case FAM_STREAM: return stream_kind(avg);
    default: return SBLAS_SPMV_ITEM_LPR;
    }
}
int64_t block_rows(int fam)
{
    switch (fam) {
    case FAM_LDS: return 8;     // SPMV_LDS_ROWS, one row per wave
    case FAM_SEG: return 16;    // four waves of four rows
    case FAM_STREAM: return 256; // ST_ROWS
    default: return 64;         // 256 lanes / 4 lanes per row
    }
}

} // namespace

extern "C" int64_t sblas_spmv_plan_classify(const int32_t *rowptr, int64_t rows, int64_t nnz, int64_t split_min,
                                            int64_t piece, int32_t *items, int64_t max_items)
{
    if (rows < 0 || nnz < 0 || (rows > 0 && !rowptr) || (items && max_items < 0)) return -1;
    if (split_min <= 0) split_min = SBLAS_SPMV_SPLIT_MIN;
    if (piece <= 0) piece = SBLAS_SPMV_SPLIT_PIECE;
    const double avg = rows > 0 ? (double)nnz / (double)rows : 0.0;
    const int gfam = family_of(avg), gkind = kind_in(gfam, avg);
    int64_t n = 0;
    auto emit = [&](int64_t r0, int64_t nr, int kind, int64_t pieces) {
        if (items && n < max_items) {
            int32_t *o = items + 4 * n;
            o[0] = (int32_t)r0, o[1] = (int32_t)nr, o[2] = kind, o[3] = (int32_t)pieces;
        }
        ++n;
    };
    for (int64_t t0 = 0; t0 < rows; t0 += TILE) {
        const int64_t t1 = t0 + TILE < rows ? t0 + TILE : rows;
        int64_t sum = 0, cnt = 0;
        for (int64_t r = t0; r < t1; ++r) {
            const int64_t len = (int64_t)rowptr[r + 1] - rowptr[r];
            if (len < 0) return -1; // row pointers must not descend
            if (len <= split_min) sum += len, ++cnt;
        }
        int fam = family_of(cnt ? (double)sum / (double)cnt : 0.0);
        // tiles of very short rows in a matrix the stream kernel takes: it ties with the lanes-per-row kernel there
        // (uniform rows of 3) and beats it on skewed rows (power-law rows averaging 3.2: 54 against 67 us when those
        // tiles went to the lanes-per-row kernel), so they stay where they are
        if (fam == FAM_LPR && gfam == FAM_STREAM) fam = FAM_STREAM;
        const int64_t br = block_rows(fam);
        // the tile's rows in runs between split rows, each run cut into kernel blocks from its first row
        for (int64_t r = t0; r < t1;) {
            const int64_t len = (int64_t)rowptr[r + 1] - rowptr[r];
            if (len > split_min) {
                emit(r, 1, SBLAS_SPMV_ITEM_SPLIT, (len + piece - 1) / piece);
                ++r;
                continue;
            }
            int64_t e = r;
            while (e < t1 && e - r < br && (int64_t)rowptr[e + 1] - rowptr[e] <= split_min) ++e;
            const double iavg = (double)((int64_t)rowptr[e] - rowptr[r]) / (double)(e - r);
            emit(r, e - r, fam == gfam ? gkind : kind_in(fam, iavg), 0);
            r = e;
        }
    }
    return n;
}
