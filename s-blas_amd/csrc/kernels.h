// kernels.h -- internal launcher interface between the kernel translation units and the C-ABI layer (capi.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "../../include/sblas_hip.h"

namespace sblas {

constexpr int MAX_REPLICAS = 16;
struct ReplicaPtrs {
    double *p[MAX_REPLICAS];
};

// SpMM stage-2 selection (SBLAS_SPMM_VARIANT, experiments and tests only).  AUTO = panel classifier, then the
// LDS-tiled / MFMA kernels on the panels that qualify and a direct kernel on the rest.
enum {
    SPMM_VARIANT_AUTO = 0,
    SPMM_VARIANT_DIRECT_DPP = 1,  // "dpp":   every panel through the row-per-wave direct kernel
    SPMM_VARIANT_DIRECT_ROWS = 2, // "rows":  every panel through the four-rows-per-wave direct kernel
    SPMM_VARIANT_LANES = 3,       // "lanes": n <= 8 keeps the lane-group kernel whatever the row length (else AUTO)
    SPMM_VARIANT_DIRECT_MERGE = 4, // "merge": every panel through the three-rows-per-wave direct kernel (128-column tiles)
    SPMM_VARIANT_MFMA = 5,        // "mfma":  LDS-tiled panels through the MFMA kernel whatever their block density
    SPMM_VARIANT_NO_MFMA = 6,     // "nomfma": never the MFMA kernel
};
constexpr int SPMM_MIN_PANEL_ROWS = 32; // smallest classified panel (the workspace tail has room for rows / 32 panels)

// Workspace layout behind the staging copy Bt ((cols + 1) x ldbt doubles): TAIL_HDR ints, TAIL_PARTS int2 (partial
// column ranges of a row block), then one int2 (column span) per panel, then one int (class) per panel.
enum { TAIL_NONFINITE = 0,    // = TAIL_STAGE_EPOCH's value when the staging pass met an Inf / NaN in B
       TAIL_STAGE_EPOCH = 1,  // epoch of the staging pass that wrote Bt
       TAIL_DIRECT_EPOCH = 2, // epoch of the classifier run that left panels to the direct kernel
       TAIL_BAND = 3,         // column span of the middle panel (band width of the matrix)
       TAIL_MFMA_EPOCH = 4,   // epoch of the classifier run that gave panels to the matrix-core kernel
       TAIL_MERGE_EPOCH = 6,  // epoch of the call whose direct panels go to the row-merging kernel (rows share column patterns)
       TAIL_MFMAD_EPOCH = 5,  // ... and some of them fall back to the DIRECT kernel when B holds a non-finite value
       TAIL_ROWS_EPOCH = 7,   // epoch of the call whose direct panels go to the four-rows-per-wave kernel (128+ staged columns)
       TAIL_HDR = 16 };
constexpr int TAIL_PARTS = 1024; // (min, max) column pairs of the column-range pass of a row block (behind the header)
enum { PANEL_DIRECT = 0, PANEL_WINDOW = 1, PANEL_MFMA_W = 2, PANEL_MFMA_D = 3,
       PANEL_CLASS_MASK = 0xff, PANEL_SHARED_ROWS = 0x100 /* flag: the panel's leading rows list the same columns */,
       PANEL_PHASE_SHIFT = 9 /* two bits: (row index where a group of three such rows starts) mod 3 */,
       PANEL_WAVE_ROWS = 0x800 /* flag: columns in runs, or row lengths far apart: a row per wave suits the panel */ };
constexpr int MFMA_MAX_WAVES = 8; // 16 rows per wave: panels of up to 128 rows (taller panels never take the MFMA kernel)
constexpr int W6_GMAX = 3;        // spmm_window6_kernel: groups of four rows per wave, 2 or 3 (template parameter)
constexpr int DPP_LONG = 4096;    // entries from which a row of the row-per-wave kernel is computed by the whole workgroup
size_t workspace_tail_bytes(int64_t rows);
unsigned long long *panel_stats_device();
hipError_t launch_spmm_mfma(hipStream_t s, int rows, int cols, const int *rowptr, const int *colidx, const double *val,
                            const double *Bt, int64_t ldbt, int n, double alpha, double beta, double *C, int64_t ldc,
                            const int2 *info, const int *tail, const int *cls, int panel_rows, int npanels, int epoch,
                            unsigned long long *stats, bool row_c, int batch, size_t lds_floor);

// The epilogue of the stage-2 kernels for a ROW-MAJOR C (element (r, j) at C[r * ldc + j]).  Every such kernel parks its
// panel of results in LDS and writes it back with alpha / beta applied; column-major C is walked with the row index
// fastest (each kernel's own loop), row-major C here with the column index fastest, so the up-to-W outputs of one panel
// row are one contiguous run of C.  at(r, j) reads the parked sum of panel row r, column j; keep(r) says whether the
// kernel owns row r.  C addresses are 64-bit.  The summation order is not touched: a row-major result is the transpose of
// the column-major one bit for bit.
__device__ __forceinline__ double c_fma(double a, double b, double c) { return fma(a, b, c); }
__device__ __forceinline__ float c_fma(float a, float b, float c) { return fmaf(a, b, c); }
template <int W, typename T, typename At, typename Keep>
__device__ __forceinline__ void store_rows_c(T *__restrict__ C, int64_t ldc, int64_t row0, int64_t col0, int prows, int nrows,
                                             int ncols, int nthreads, T alpha, T beta, At at, Keep keep)
{
    for (int idx = threadIdx.x; idx < W * prows; idx += nthreads) {
        const int j = idx % W, r = idx / W;
        if (r < nrows && j < ncols && keep(r)) {
            T *dst = C + (row0 + r) * ldc + (col0 + j);
            const T sres = alpha * at(r, j);
            *dst = (beta == T(0)) ? sres : c_fma(beta, *dst, sres);
        }
    }
}

// The same epilogue in two steps for the 1024-thread LDS-tiled kernel and its 64-column halves, either layout of C:
// panel_c_fetch issues EVERY old-C load of the thread into registers (none at all when beta == 0) and returns without
// using them, so the kernel can put barriers and the parking of its sums between the two steps and pay one memory
// round trip per panel instead of one per trip; panel_c_store applies them.  The thread -> (row, column) map is fixed
// and needs no division: row-major C as store_rows_c<64> with 1024 threads (a wave on the 64 columns of one row, rows
// 16 apart per trip); column-major C with a half-wave on 32 consecutive rows of one column (trip i: rows 32 (i / 2) ..,
// column 32 (i % 2) + tid / 32).  RMAX / 16 trips cover 64 columns x RMAX rows in both; trips past nrows are dead for
// the whole workgroup.  Same fma(beta, old, alpha * sum) as store_rows_c.
template <bool RC> __device__ __forceinline__ void panel_c_map(int i, int &r, int &j)
{
    const int tid = (int)threadIdx.x;
    if (RC) r = (tid >> 6) + 16 * i, j = tid & 63;
    else r = 32 * (i >> 1) + (tid & 31), j = 32 * (i & 1) + (tid >> 5);
}
template <bool RC> __device__ __forceinline__ int64_t panel_c_index(int64_t ldc, int64_t row0, int64_t col0, int r, int j)
{
    return RC ? (row0 + r) * ldc + (col0 + j) : (col0 + j) * ldc + (row0 + r);
}
template <bool RC, int TRIPS>
__device__ __forceinline__ void panel_c_fetch(const double *__restrict__ C, int64_t ldc, int64_t row0, int64_t col0, int nrows,
                                              int ncols, double beta, double (&old)[TRIPS])
{
#pragma unroll
    for (int i = 0; i < TRIPS; ++i) old[i] = 0.0;
    if (beta == 0.0) return; // C is not read
#pragma unroll
    for (int i = 0; i < TRIPS; ++i) {
        int r, j;
        panel_c_map<RC>(i, r, j);
        if (r < nrows && j < ncols) old[i] = C[panel_c_index<RC>(ldc, row0, col0, r, j)];
    }
}
template <bool RC, int TRIPS, typename At>
__device__ __forceinline__ void panel_c_store(double *__restrict__ C, int64_t ldc, int64_t row0, int64_t col0, int nrows,
                                              int ncols, double alpha, double beta, const double (&old)[TRIPS], At at)
{
    double sum[TRIPS]; // (read ahead of the stores: one LDS round trip, not one per trip)
#pragma unroll
    for (int i = 0; i < TRIPS; ++i) {
        int r, j;
        panel_c_map<RC>(i, r, j);
        sum[i] = (r < nrows && j < ncols) ? at(r, j) : 0.0;
    }
#pragma unroll
    for (int i = 0; i < TRIPS; ++i) {
        int r, j;
        panel_c_map<RC>(i, r, j);
        if (r < nrows && j < ncols) {
            const double sres = alpha * sum[i];
            C[panel_c_index<RC>(ldc, row0, col0, r, j)] = (beta == 0.0) ? sres : c_fma(beta, old[i], sres);
        }
    }
}

// Workgroups are dealt round-robin over the 8 XCDs (b and b+8 share one).  Give every XCD one contiguous
// range of panels so that neighbouring panels -- which read overlapping Bt rows -- share an L2 (speed only;
// any placement is correct).  Bijective for every panel count.
__device__ __forceinline__ int xcd_contiguous_panel(int b, int npanels)
{
    const int xcd = b & 7, idx = b >> 3;
    const int q = npanels >> 3, r = npanels & 7;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

// Experiment / test switches, read from the environment once (spmm_rule.cpp); options_reload() re-reads them.
struct Options {
    int spmm_variant = SPMM_VARIANT_AUTO;
    char spmv_variant[16] = {0};          // "" = auto
    bool tier16 = true, tier32 = true;    // staged widths 16 / 32 for n <= 16 / 32 (SBLAS_SPMM_MIN_LDBT: 0 = both, 64 = neither: the 64-column copy)
    unsigned long long max_bt_bytes = 0xffffffffull; // SBLAS_SPMM_MAX_BT_BYTES (tests of the column-chunk loop)
    int direct_lds = -1;                  // SBLAS_DIRECT_LDS
    int direct_map = -1;                  // SBLAS_DIRECT_MAP: 1 interleave, 0 contiguous, -1 by span
    int stage_range = -1;                 // SBLAS_STAGE_RANGE: stage only the rows of B a row block refers to (-1: when the saved staging traffic outweighs the column-range pass)
    int direct_merge = 1;                 // SBLAS_DIRECT_MERGE: 128-column direct panels through the row-merging kernel
    double rows8_min_avg = 256.0;         // SBLAS_ROWS8_MIN_AVG
    float window_density = 0.42f;         // SBLAS_WINDOW_DENSITY: the LDS-tiled kernel's bar, in nonzeros per spanned column of a 16-row slice of a panel
    int panel_rows = 0, panel_groups = 0; // SBLAS_SPMM_PANEL_ROWS
    // SBLAS_TUNE=a,b,c,d: four integers for A/B runs, each parsed once (options_parse) into everything it switches
    int lanes_copies = 1;                 // a = 2 | 4: copies of a Bt row in the narrow LDS tile (8 columns: 2 or 4; 16 columns: 2, which also caps the groups per wave at two)
    size_t mfma_lds_floor = 0;            // 0 < a <= 160 KiB: least dynamic LDS of the matrix-core kernel (occupancy)
    bool one_half = false;                // b = 1: one 64-column half per LDS-tiled workgroup at 128+ staged columns (and three groups per wave allowed)
    int rowlen_bar = 0;                   // b > 1: the classifier's average-row-length bar at every width (0: the measured ones)
    int mfma_batch64 = 2;                 // b = 3 | 4: operand blocks per stage of the matrix-core kernel at 64 staged columns
    int mfma_batch128 = 2;                // b = 1: ... at 128+ staged columns
    int dpp_long = DPP_LONG;              // c > 0: entries from which the row-per-wave kernel splits a row over its sixteen waves
    bool lanes32_one_lane = false;        // d = 1: 32 columns with one lane per entry and one group per wave
    int rows_waves = 0;                   // d = 4 | 8 | 16: waves per workgroup of the four-rows kernel (0: by row length)
    bool validate = false;                // SBLAS_VALIDATE=1: every SpMM / SpMV call checks the CSR contents first (synchronises; debugging)
    float mfma_min_fill = -1.0f;          // SBLAS_MFMA_MIN_FILL: block fill from which a panel takes the MFMA kernel (< 0: built-in rule)
};
const Options &options();
void options_reload();
int compute_units(); // of the current device (kernels.hip)
int next_epoch();    // tags one call's classifier verdicts and one staging pass (see classify_panel)
void raise_dynamic_lds(const void *fn, size_t bytes);

// A per-matrix plan (capi.hip: sblas_hip_spmm_plan_*): the panel verdicts of one (A, staged width) pair kept in a device
// buffer of the plan's own (same layout as the workspace tail), and what the host learned from them once -- which
// stage-2 kernels have panels at all, the matrix-wide votes, a row block's column range.
struct PlanView {
    int *tail = nullptr;        // TAIL_HDR ints + TAIL_PARTS int2 + one int2 + one int per panel (device)
    int epoch = 0;              // the classifier epoch the verdicts carry
    int info_rows = 0, groups = 0;
    long n_window = 0, n_direct = 0, n_mfma_w = 0, n_mfma_d = 0; // panels per class after the votes
    bool merge = false;         // the call's direct panels go to the row-merging kernel
    bool four_rows = false;     // ... to the four-rows-per-wave kernel (128+ staged columns)
    bool use_range = false;     // stage only the column range [lo, hi] of B
    int nparts = 0;
    // a split plan's long rows (sblas_hip_spmm_plan_create_split; all null / 0 otherwise): one bit per row, the pieces
    // and the split rows (split_rows) and one partial row of ldbt doubles per piece, in the plan's device buffer
    const unsigned *split_bits = nullptr;
    const int4 *pieces = nullptr, *srows = nullptr;
    double *partial = nullptr;
    int64_t n_pieces = 0, n_split = 0, split_nnz = 0;
};
size_t plan_tail_bytes(int64_t rows);

// The split rows of both plans (sblas_spmm_split_classify, sblas_hip_spmv_plan_create): the rows that split(row, len)
// selects, cut into pieces of at most `piece` consecutive nonzeros.  Records of four int32: first the pieces {row, first
// nonzero, end, partial slot} with slots 0, 1, .. in row order (the pieces of a row consecutive, in CSR order), then one
// record per split row {row, first slot, pieces, -1}.  Writes the records below max_out when out is not null; returns the
// number of records, or -1 when the row pointers descend.
template <typename Split>
int64_t split_rows(const int32_t *rowptr, int64_t rows, int64_t piece, Split split, int32_t *out, int64_t max_out)
{
    int64_t n_pieces = 0, n_split = 0;
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t len = (int64_t)rowptr[r + 1] - rowptr[r];
        if (len < 0) return -1;
        if (split(r, len)) ++n_split, n_pieces += (len + piece - 1) / piece;
    }
    if (!out) return n_pieces + n_split;
    int64_t slot = 0, k = n_pieces; // pieces at [0, n_pieces), split rows behind them
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t b = rowptr[r], e = rowptr[r + 1];
        if (!split(r, e - b)) continue;
        if (k < max_out) {
            int32_t *o = out + 4 * k;
            o[0] = (int32_t)r, o[1] = (int32_t)slot, o[2] = (int32_t)((e - b + piece - 1) / piece), o[3] = -1;
        }
        ++k;
        for (int64_t pb = b; pb < e; pb += piece, ++slot) {
            if (slot >= max_out) continue;
            int32_t *o = out + 4 * slot;
            o[0] = (int32_t)r, o[1] = (int32_t)pb, o[2] = (int32_t)(pb + piece < e ? pb + piece : e), o[3] = (int32_t)slot;
        }
    }
    return n_pieces + n_split;
}

// What one column chunk of an SpMM call does before stage 2, decided in one place (spmm_step): how B is staged, whether
// stage 2 reads panel verdicts and where they come from, and the panel geometry the classifier and stage 2 agree on.
enum {
    STAGE_CALLER = 0,  // Bt comes from the caller (sblas_hip_spmm_csr_rowmajorB_f64_i32)
    STAGE_FULL = 1,    // the whole of B
    STAGE_FUSED = 2,   // the whole of B, the panel classifier in the same launch
    STAGE_RANGE = 3,   // the rows of B a row block's nonzeros refer to, after a column-range pass
    STAGE_PLANNED = 4, // the whole of B or the plan's column range, stamped into the plan's header
};
enum {
    VERDICTS_NONE = 0,     // none: a direct kernel takes every panel
    VERDICTS_STAGING = 1,  // the staging launch classifies (fused, or in the column-range pass)
    VERDICTS_SEPARATE = 2, // a classifier launch of its own ahead of stage 2
    VERDICTS_EARLIER = 3,  // an earlier column chunk of the same range-staged call classified
    VERDICTS_PLAN = 4,     // the plan's
};
struct SpmmStep {
    int staging = STAGE_FULL, verdicts = VERDICTS_NONE;
    int64_t ldbt = 0;
    int info_rows = 1, groups = 2, npanels = 0; // (1, 2, 0: nothing classified)
    int epoch = 0;                              // of the verdicts, or of stage 2 alone
    bool plannable = false;                     // a plan may keep the verdicts (sblas_hip_spmm_plan_create)
    const PlanView *pv = nullptr;
};
// pv: the call's plan, when it was made at this ldbt; prev: the call's previous column chunk
SpmmStep spmm_step(int rows, int cols, int64_t nnz, int64_t ldbt, const PlanView *pv, const SpmmStep &prev = SpmmStep(),
                   bool caller_staged = false);
// The classifier's thresholds (classify_args): the longest row a windowed panel may hold (32-bit buffer offsets inside a
// wave's rows), nonzeros per spanned column and per row a panel needs for the LDS-tiled kernel, the block fill from which
// it takes the matrix cores (> 1: never), what to probe for the direct kernels' sake (bit 0 row-merging, bit 1 row per wave).
struct ClassifyArgs {
    int max_row_len;
    float min_density, min_rowlen, mfma_min_fill;
    int merge_probe;
};
ClassifyArgs classify_args(int panel_rows, int64_t ldbt);
int range_parts(int64_t nnz); // (min, max) pairs of the column-range pass of a row block

// What stage 2 of a chunk launches, in launch order (spmm_stage2, spmm_rule.cpp: DESIGN.md 3's selection table);
// launch_spmm_rowpanel carries it out and decides nothing.  Template arguments are spelled as the kernels take them.
enum { TILED_NONE = 0, TILED_WINDOW6 = 1 /* spmm_window6_kernel<G, NH> */, TILED_LANES = 2 /* spmm_lanes_kernel<NC, CP, G, LPE> */ };
struct SpmmStage2 {
    // 1. the LDS-tiled kernel on the panels that qualify
    int tiled = TILED_NONE;
    int g = 0;                  // groups of four rows per wave (either kernel)
    int nh = 0, grid_y = 0;     // spmm_window6_kernel: 64-column halves per workgroup, workgroups along the columns
    int nc = 0, cp = 0, lpe = 0; // spmm_lanes_kernel: staged columns, copies of a Bt row in the tile, lanes per entry
    // 2. the matrix-core kernel on its panels (spmm_mfma_kernel)
    bool mfma = false;
    int mfma_batch = 0;         // operand blocks per stage
    size_t mfma_lds_floor = 0;  // least dynamic LDS (0: what the panel needs)
    // 3. the direct kernels on the rest, in this order; classified calls at 128+ columns launch up to three of them and
    // the device-side vote picks (voted), everywhere else exactly one runs
    bool four_rows = false;     // spmm_direct_rows_kernel<WV>
    int rows_waves = 0, voted = 0;
    bool merge = false;         // spmm_direct_merge_kernel
    int dpp = 0;                // spmm_direct_dpp_kernel<GROUPS>: 1, 2 or 4 (0: not launched)
    size_t dpp_pad = 0;         // ... its dynamic LDS pad
    int dpp_long = 0;           // ... entries from which the whole workgroup computes a row
    int narrow = 0;             // spmm_rowpanel_narrow_kernel<8 | 16 | 32> (0: not launched)
    bool rows8 = false;         // spmm_rows8_kernel
    int interleave = -1;        // panel map of the direct kernels: 1 interleave, 0 contiguous, -1 by the classifier's span
    // 4. a split plan: the direct kernels above in their SKIP instantiations, then spmm_split_piece_kernel<GROUPS> + fold
    bool skip = false;
    int split_groups = 0;
};
SpmmStage2 spmm_stage2(const SpmmStep &st, int rows, int cols, int64_t nnz, int n);
// Layouts of the dense operands: row_b = B is row-major (cols x n, B[k * ldb + j]; only the staging launchers read B),
// row_c = C is row-major (rows x n, C[r * ldc + j]; the stage-2 epilogues, the scale and the merge kernels).
hipError_t launch_stage(hipStream_t s, const SpmmStep &st, int rows, int64_t cols, int64_t nnz, const int *rowptr,
                        const int *colidx, int64_t n, const double *B, int64_t ldb, double *Bt, bool row_b);
hipError_t launch_spmm_rowpanel(hipStream_t s, const SpmmStep &st, int rows, int cols, int64_t nnz, const int *rowptr,
                                const int *colidx, const double *val, const double *Bt, int n, double alpha, double beta,
                                double *C, int64_t ldc, bool row_c);
// the verdicts of the step's classifier into pv; cls_out (optional): one class word per panel, as the host read them
hipError_t plan_build(hipStream_t s, const SpmmStep &st, int rows, int cols, int64_t nnz, const int *rowptr, const int *colidx,
                      PlanView *pv, std::vector<int> *cls_out = nullptr);
hipError_t launch_dense_to_rowmajor(hipStream_t s, int64_t cols, int64_t n, const double *B, int64_t ldb,
                                    double *Bt, int64_t ldbt, bool row_b);
hipError_t launch_scale(hipStream_t s, int64_t rows, int64_t n, double beta, double *C, int64_t ldc, bool row_c);
hipError_t validate_csr(hipStream_t s, int64_t rows, int64_t cols, int64_t nnz, const int *rowptr, const int *colidx, int *bad);
hipError_t panel_stats(unsigned long long out[4], bool reset);
hipError_t launch_spmv(hipStream_t s, int rows, int cols, int64_t nnz, const int *rowptr, const int *colidx,
                       const double *val, const double *x, double alpha, double beta, double *y);
// The SpMV kernel rule (spmv_plan.cpp): the SBLAS_SPMV_ITEM_* kind for rows of `avg` nonzeros on average -- launch_spmv's
// choice for a whole matrix, the plan's for a tile.  family >= 0 (LPR, STREAM4096, SEG or LDS_S2: the first kind of a
// kernel family) asks for the kind inside that family, whatever family avg itself falls in.
int spmv_kind(double avg, int family = -1);
// Rows per block of the instantiations spmv_kind picks (spmv_kernels.hip); a plan's work item is at most one block.
constexpr int SPMV_LPR = 4;                   // lanes-per-row kernel: 4 lanes per row ...
constexpr int SPMV_LPR_ROWS = 256 / SPMV_LPR; // ... 64 rows per 256-thread block
constexpr int ST_ROWS = 256;                  // stream kernel: a row per thread
constexpr int SPMV_SEG_R = 4;                 // segmented kernel: rows per wave ...
constexpr int SPMV_SEG_ROWS = 4 * SPMV_SEG_R; // ... 16 rows per four-wave block
constexpr int SPMV_LDS_ROWS = 8;              // LDS-window kernel: a row per wave, eight waves
// A per-matrix SpMV plan (capi.hip: sblas_hip_spmv_plan_*).  Work items of the kernel classes, grouped by class
// (items + off[k] .. items + off[k + 1]; int4 {first row, row count, window lo, window hi}; the window only for the
// LDS-window classes), the split-row records (split_rows) and one partial sum per piece, all in the plan's device buffer.
constexpr int SPMV_ITEM_KERNELS = SBLAS_SPMV_ITEM_SPLIT; // the kinds SBLAS_SPMV_ITEM_LPR .. _LDS_S7 have a kernel each
struct SpmvPlanView {
    int4 *items = nullptr;
    int64_t off[SPMV_ITEM_KERNELS + 1] = {0};
    const int4 *pieces = nullptr, *srows = nullptr;
    double *partial = nullptr;
    int64_t n_pieces = 0, n_split = 0;
    bool as_unplanned = false; // every item is of one lanes-per-row / stream / segmented class: launch_spmv's launch
};
hipError_t spmv_plan_windows(hipStream_t s, int n, int4 *items, const int *rowptr, const int *colidx);
hipError_t launch_spmv_planned(hipStream_t s, int cols, const SpmvPlanView &pv, const int *rowptr, const int *colidx,
                               const double *val, const double *x, double alpha, double beta, double *y);
hipError_t launch_axpby(hipStream_t s, int64_t n, double alpha, const double *x, double beta, double *y);
void kernel_events_enable(bool on);
hipError_t kernel_events_last_ms(float *ms);
hipError_t launch_merge_rowblocks(hipStream_t s, int64_t M, int64_t N, int g, const double *const *src,
                                  const int64_t *start, const int64_t *nrows, double alpha, double beta, double *C,
                                  int64_t ldc, bool row_c);

// typed_kernels.hip: the value / index types besides <int32, fp64> (reference utility.h:302-316)
enum { VT_F64 = 0, VT_F32 = 1 };
enum { IT_I32 = 0, IT_I64 = 1 };
int64_t typed_spmm_ldbt(int64_t n);
size_t typed_spmm_workspace(int vt, int64_t cols, int64_t n);
hipError_t launch_typed_spmm(hipStream_t s, int vt, int it, int64_t rows, int64_t cols, int64_t nnz, const void *rowptr,
                             const void *colidx, const void *val, const void *B, int64_t ldb, int64_t n, double alpha,
                             double beta, void *C, int64_t ldc, void *ws, bool row_b, bool row_c);
hipError_t launch_typed_spmv(hipStream_t s, int vt, int it, int64_t rows, const void *rowptr, const void *colidx,
                             const void *val, const void *x, double alpha, double beta, void *y);
hipError_t launch_typed_axpby(hipStream_t s, int vt, int64_t n, double alpha, const void *x, double beta, void *y);
hipError_t launch_typed_sum_replicas(hipStream_t s, int vt, void *const *bufs, int g, int64_t n);
hipError_t launch_typed_merge_rowblocks(hipStream_t s, int vt, int64_t M, int64_t N, int g, const void *const *src,
                                        const int64_t *start_row, const int64_t *num_rows, double alpha, double beta,
                                        void *C, int64_t ldc, bool row_c);

} // namespace sblas
