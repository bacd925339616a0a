// spmv_plan.cpp -- the SpMV kernel rule (spmv_kind) and the host half of the SpMV plan (sblas_hip_spmv_plan_*): the
// row-length classifier that cuts a matrix into work items.  Pure functions of the row pointers; no GPU call in this
// file, so it is testable on a CPU box.
//
// The unplanned launcher (launch_spmv, spmv_kernels.hip) picks ONE kernel for the whole matrix from nnz / rows, by
// spmv_kind below.  Here the rows are taken in tiles of 256 (the stream kernel's block; every other kernel's block --
// 64, 16 and 8 rows -- divides it) and each tile is classified by the average length of its rows, by the same rule.  A
// tile whose kernel family is the one the launcher picks for the whole matrix takes exactly the launcher's
// instantiation, so a matrix whose tiles all agree is computed by the same kernel, block for block, as the unplanned
// call.  A tile of another family takes the instantiation its own rows ask for.  A row longer than `split_min` becomes an
// item of its own and is cut into pieces of `piece` nonzeros that run on as many workgroups.
#include <stdint.h>
#include "../../include/sblas_hip.h"
#include "kernels.h"

namespace sblas {

int spmv_kind(double avg, int family)
{
    if (family < 0) {
        // long rows: x window in LDS (bench matrix: 70-73 us vs 82-85 us for the lanes-per-row kernel); a block whose
        // rows span more than the LDS window degrades to global gathers by itself
        if (avg > 96.0) family = SBLAS_SPMV_ITEM_LDS_S2;
        // medium rows: R rows per wave, segmented (Queen-like rows, 73 per row: 232 us vs 395 us; banded synthetic rows
        // of 36 / 72 / 90: 122 / 266 / 351 us vs 150 / 339 / 375 us for the lanes-per-row kernel)
        else if (avg > 64.0) family = SBLAS_SPMV_ITEM_SEG;
        // short and medium rows (2.5 < avg <= 64): 256 rows per block streamed through LDS, in runs of up to 6144
        // products (stencil-like rows of 7 / 13 / 27: 108 / 177 / 344 us vs 143 / 277 / 498 us for the lanes-per-row and
        // segmented kernels; banded-random rows of 14 / 20 / 28 / 36 / 48: 46 / 62 / 85 / 116 / 161 vs 49 / 71 / 94 /
        // 128 / 194; 1 M banded rows of 55 / 70: 207 / 256 us vs 250 / 281 us segmented; Queen-like rows of 73: 251 vs
        // 256 us).  Rows beyond 96 take the kernel's slow path (a wave per row), so it stops where a spread of row
        // lengths starts to reach that: Poisson rows of 60 on average tie, of 70 lose 4 %, of 80 7 %, of 90 27 % -- the
        // launcher only knows the average.  Round 3 (four blocks per CU for short rows): 2 M uniform rows of 3 / 5: 35.9 /
        // 40.0 us against 34.6-36.1 / 50.0 us for the lanes-per-row kernel, power-law rows averaging 3.2: 55.7 against
        // 67 us -- the stream form from 2.5 per row on (round 2: from 5).
        else if (avg > 2.5) family = SBLAS_SPMV_ITEM_STREAM4096;
        else family = SBLAS_SPMV_ITEM_LPR;
    }
    if (family == SBLAS_SPMV_ITEM_LDS_S2) {
        // slices in flight per row: ~1.3-1.5 x the row length in 64-lane slices (600 k banded rows of 100 / 130 / 160 /
        // 200 / 260, band +-2000: S = 2 / 3 / 3 / 4 / 7 take 273 / 307 / 315 / 360 / 433 us against 329 / 337 / 345 / 360
        // / 451 us with S = 4 throughout; the same order on a +-20000 band, tools/spmv_rowlen_sweep.py)
        if (avg <= 115.0) return SBLAS_SPMV_ITEM_LDS_S2;
        if (avg <= 180.0) return SBLAS_SPMV_ITEM_LDS_S3;
        if (avg <= 230.0) return SBLAS_SPMV_ITEM_LDS_S4;
        return SBLAS_SPMV_ITEM_LDS_S7;
    }
    if (family == SBLAS_SPMV_ITEM_STREAM4096) {
        // the LDS capacity that gives a block of average rows the fewest runs; a tie goes to the smaller one
        const double per_block = avg * ST_ROWS;
        const int runs4 = (int)((per_block + 4095.0) / 4096.0), runs6 = (int)((per_block + 6143.0) / 6144.0);
        return runs4 <= runs6 ? SBLAS_SPMV_ITEM_STREAM4096 : SBLAS_SPMV_ITEM_STREAM6144;
    }
    return family; // LPR, SEG: one instantiation each
}

} // namespace sblas

namespace {

constexpr int64_t TILE = sblas::ST_ROWS;

// a kind's kernel family, named by its first kind (LPR, STREAM4096, SEG, LDS_S2), and the rows of its blocks
int family_of(int kind)
{
    if (kind == SBLAS_SPMV_ITEM_STREAM6144) return SBLAS_SPMV_ITEM_STREAM4096;
    return kind > SBLAS_SPMV_ITEM_LDS_S2 ? SBLAS_SPMV_ITEM_LDS_S2 : kind;
}
int64_t block_rows(int family)
{
    switch (family) {
    case SBLAS_SPMV_ITEM_LDS_S2: return sblas::SPMV_LDS_ROWS;
    case SBLAS_SPMV_ITEM_SEG: return sblas::SPMV_SEG_ROWS;
    case SBLAS_SPMV_ITEM_STREAM4096: return sblas::ST_ROWS;
    default: return sblas::SPMV_LPR_ROWS;
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
    const int gkind = sblas::spmv_kind(avg), gfam = family_of(gkind);
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
        int fam = family_of(sblas::spmv_kind(cnt ? (double)sum / (double)cnt : 0.0));
        // tiles of very short rows in a matrix the stream kernel takes: it ties with the lanes-per-row kernel there
        // (uniform rows of 3) and beats it on skewed rows (power-law rows averaging 3.2: 54 against 67 us when those
        // tiles went to the lanes-per-row kernel), so they stay where they are
        if (fam == SBLAS_SPMV_ITEM_LPR && gfam == SBLAS_SPMV_ITEM_STREAM4096) fam = SBLAS_SPMV_ITEM_STREAM4096;
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
            emit(r, e - r, fam == gfam ? gkind : sblas::spmv_kind(iavg, fam), 0);
            r = e;
        }
    }
    return n;
}
