// spmm_rule.cpp -- the host half of an SpMM column chunk: the experiment switches (Options), what the chunk does before
// stage 2 (spmm_step) and which stage-2 kernels it launches, with which template arguments, in which order
// (spmm_stage2: the selection table of DESIGN.md 3).  Pure functions of the call's sizes, the plan's counts and the
// switches; no GPU call in this file, so it is testable on a CPU box (sblas_spmm_rule_describe, tests/test_spmm_rule_host.py).
//
// kernels.hip carries the decisions out: launch_stage and launch_spmm_rowpanel hold the launch sites and decide nothing.
// options_parse and spmm_stage2 are the only places that name a tuning switch of stage 2; the thresholds, with the
// measurements behind them, are the functions in between.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include "../../include/sblas_hip.h"
#include "kernels.h"

namespace sblas {

// ---------------------------------------------------------------------------------------------
// Experiment / test switches.  The environment is read ONCE (first launch) into this struct; tests that change a
// switch inside one process call sblas_hip_debug_reload_env() afterwards.  Nothing here changes results.
// ---------------------------------------------------------------------------------------------
static Options g_options;
static std::atomic<bool> g_options_loaded{false};
static std::mutex g_options_mu;
static void options_parse(Options &o)
{
    o = Options{};
    const char *e;
    if ((e = getenv("SBLAS_SPMM_VARIANT")) && *e) {
        if (!strcmp(e, "dpp")) o.spmm_variant = SPMM_VARIANT_DIRECT_DPP;
        else if (!strcmp(e, "rows")) o.spmm_variant = SPMM_VARIANT_DIRECT_ROWS;
        else if (!strcmp(e, "lanes")) o.spmm_variant = SPMM_VARIANT_LANES;
        else if (!strcmp(e, "merge")) o.spmm_variant = SPMM_VARIANT_DIRECT_MERGE;
        else if (!strcmp(e, "mfma")) o.spmm_variant = SPMM_VARIANT_MFMA;
        else if (!strcmp(e, "nomfma")) o.spmm_variant = SPMM_VARIANT_NO_MFMA;
    }
    if ((e = getenv("SBLAS_SPMV_VARIANT")) && *e && strcmp(e, "auto")) {
        strncpy(o.spmv_variant, e, sizeof o.spmv_variant - 1);
    }
    if ((e = getenv("SBLAS_SPMM_MIN_LDBT")) && *e) o.tier16 = o.tier32 = atoi(e) < 64;
    if ((e = getenv("SBLAS_SPMM_MAX_BT_BYTES")) && *e) {
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v >= 4096 && v < 0xffffffffull) o.max_bt_bytes = v;
    }
    if ((e = getenv("SBLAS_DIRECT_LDS")) && *e) o.direct_lds = atoi(e);
    if ((e = getenv("SBLAS_DIRECT_MERGE")) && *e) o.direct_merge = atoi(e);
    if ((e = getenv("SBLAS_STAGE_RANGE")) && *e) o.stage_range = atoi(e);
    if ((e = getenv("SBLAS_DIRECT_MAP")) && *e) o.direct_map = !strcmp(e, "interleave") ? 1 : !strcmp(e, "contiguous") ? 0 : -1;
    if ((e = getenv("SBLAS_ROWS8_MIN_AVG")) && *e) o.rows8_min_avg = atof(e);
    if ((e = getenv("SBLAS_WINDOW_DENSITY")) && *e) o.window_density = (float)atof(e);
    if ((e = getenv("SBLAS_SPMM_PANEL_ROWS")) && *e) { /* "<rows>" or "<rows>,<groups>" */
        o.panel_rows = atoi(e);
        o.panel_groups = strchr(e, ',') ? atoi(strchr(e, ',') + 1) : 0;
    }
    if ((e = getenv("SBLAS_MFMA_MIN_FILL")) && *e) o.mfma_min_fill = (float)atof(e);
    if ((e = getenv("SBLAS_VALIDATE")) && *e) o.validate = atoi(e) != 0;
    if ((e = getenv("SBLAS_TUNE")) && *e) { /* "a,b,c,d" (or "a:b:c:d"): integers for kernel experiments, 0 = default */
        char buf[96];
        strncpy(buf, e, sizeof buf - 1);
        buf[sizeof buf - 1] = 0;
        for (char *c = buf; *c; ++c)
            if (*c == ':') *c = ',';
        int a = 0, b = 0, c = 0, d = 0;
        sscanf(buf, "%d,%d,%d,%d", &a, &b, &c, &d);
        // One integer switches several things, each at another staged width or in another kernel; this is the one place
        // that says which ("Runtime switches").
        if (a == 2 || a == 4) o.lanes_copies = a;                      // narrow LDS tile; 2 also caps the groups at 16 columns
        if (a > 0 && a <= 160 * 1024) o.mfma_lds_floor = (size_t)a;    // matrix-core kernel (a floor: small values change nothing)
        o.one_half = b == 1;                                           // LDS-tiled kernel at 128+ columns
        if (b > 1) o.rowlen_bar = b;                                   // classifier, every width: threshold sweeps
        if (b == 3 || b == 4) o.mfma_batch64 = b;                      // matrix-core kernel, 64 columns
        if (b == 1) o.mfma_batch128 = 1;                               // matrix-core kernel, 128+ columns
        if (c > 0) o.dpp_long = c;                                     // row-per-wave kernel: A/B runs of the long-row split
        o.lanes32_one_lane = d == 1;                                   // narrow LDS-tiled kernel at 32 columns
        if (d == 4 || d == 8 || d == 16) o.rows_waves = d;             // four-rows kernel: pins the workgroup size
    }
}
const Options &options()
{
    if (!g_options_loaded.load(std::memory_order_acquire)) {
        std::lock_guard<std::mutex> lock(g_options_mu);
        if (!g_options_loaded.load(std::memory_order_relaxed)) {
            options_parse(g_options);
            g_options_loaded.store(true, std::memory_order_release);
        }
    }
    return g_options;
}
void options_reload()
{
    std::lock_guard<std::mutex> lock(g_options_mu);
    options_parse(g_options);
    g_options_loaded.store(true, std::memory_order_release);
}

static std::atomic<int> g_epoch{1};
int next_epoch() { return g_epoch.fetch_add(1, std::memory_order_relaxed); }

// ---------------------------------------------------------------------------------------------
// Panel geometry: the panel height and the groups per wave that the classifier and the stage-2 kernels of a call agree on.
// ---------------------------------------------------------------------------------------------
// Sixth generation, one workgroup per CU at a time: the groups per wave (2 or 3) and the panel height (a multiple of
// the rows of a wave) that minimise rounds x (height + per-tile fixed cost).
static void gen6_plan(int rows, int ncu, int &info_rows, int &gen6_g, int gmax = W6_GMAX)
{
    int best = 128;
    long best_cost = -1;
    gen6_g = 2;
    for (int g = 2; g <= gmax; ++g)
        for (int r = 12 * 4 * g; r >= 4 * 4 * g; r -= 4 * g) {
            const long panels = ((long)rows + r - 1) / r;
            // measured on the bench matrix: three groups per wave cost ~15 % more per row
            const long cost = ((panels + ncu - 1) / ncu) * (long)(r + 40) * (g == 3 ? 23 : 20);
            if (best_cost < 0 || cost < best_cost) {
                best_cost = cost;
                best = r;
                gen6_g = g;
            }
        }
    info_rows = best;
    const Options &opt = options();
    if (opt.panel_rows > 0) { /* experiments */
        const int r = opt.panel_rows, g = opt.panel_groups ? opt.panel_groups : (r % 12 == 0 && r > 128 ? 3 : 2);
        if (g >= 2 && g <= gmax && r >= SPMM_MIN_PANEL_ROWS && r <= 48 * g && r % (4 * g) == 0) { // (workspace: a verdict per 32 rows)
            info_rows = r;
            gen6_g = g;
        }
    }
}

// Panel height of the narrow LDS-tiled kernel: twelve consumer waves of G groups of four rows; G is capped by the
// registers NC accumulators per group take (8 columns: 3, 16 and 32: 1).
static void lanes_plan(int rows, int ldbt, int ncu, int &info_rows, int &groups)
{
    const Options &opt = options();
    const int gmax = ldbt <= 8 ? 3 : ldbt <= 16 ? (opt.lanes_copies == 2 ? 2 : 3) : opt.lanes32_one_lane ? 1 : 2;
    long best_cost = -1;
    info_rows = 48;
    groups = 1;
    // 8 columns: one group of rows per wave, two workgroups per CU (see spmm_lanes_kernel); SBLAS_SPMM_PANEL_ROWS overrides
    for (int g = 1; g <= gmax && ldbt > 8; ++g)
        for (int r = 12 * 4 * g; r >= 4 * 4 * g; r -= 4 * g) {
            if (r < SPMM_MIN_PANEL_ROWS) continue;
            const long panels = ((long)rows + r - 1) / r;
            const long cost = ((panels + ncu - 1) / ncu) * (long)(r + 40);
            if (best_cost < 0 || cost < best_cost) {
                best_cost = cost;
                info_rows = r;
                groups = g;
            }
        }
    if (opt.panel_rows > 0) { /* experiments */
        const int r = opt.panel_rows, g = opt.panel_groups ? opt.panel_groups : 1;
        if (g >= 1 && g <= gmax && r >= SPMM_MIN_PANEL_ROWS && r <= 48 * g && r % (4 * g) == 0) {
            info_rows = r;
            groups = g;
        }
    }
}

// the panel height the classifier and the stage-2 kernels of a call agree on
static void panel_plan(int rows, int64_t ldbt, int ncu, int &info_rows, int &groups)
{
    if (ldbt < 64) lanes_plan(rows, (int)ldbt, ncu, info_rows, groups);
    // (128+ staged columns: two column halves per workgroup, whose accumulators leave room for two groups per wave)
    // (... and so does SBLAS_SPMM_VARIANT=mfma at 64 columns: the matrix-core kernel takes panels of up to 16 rows x
    //  MFMA_MAX_WAVES, and three groups per wave would give 132- / 144-row panels it silently leaves alone: ADVICE r2)
    else gen6_plan(rows, ncu, info_rows, groups,
                   ((ldbt >= 128 && !options().one_half) || options().spmm_variant == SPMM_VARIANT_MFMA) ? 2 : W6_GMAX);
}

// ---------------------------------------------------------------------------------------------
// The classifier's thresholds.
// ---------------------------------------------------------------------------------------------
// Nonzeros a panel must hold per column of its span to take the LDS-tiled kernel: every row of a B tile it loads is then
// used that many times on average.  0.42 per 16 rows = 2.5 uses for a 96-row panel -- measured on banded rows, 1 M
// rows, N = 64 (tools/spmm_shapes.py banded:ROWS:PERROW:HALFBAND with SBLAS_WINDOW_DENSITY): at 1.4 uses the direct
// kernel wins by 36 %, at 2.1-2.4 the two are within 5 %, from 2.75 on the LDS-tiled kernel wins (6 % ... 70 % at 6 uses,
// where round 1's bar stood).
static float window_min_density(int panel_rows) { return options().window_density * (float)panel_rows / 16.0f; }
// Nonzeros per row a panel must average to take the LDS-tiled kernel.  Measured on banded rows (tools/spmm_shapes.py
// banded:ROWS:PERROW:HALFBAND, 1 M rows) against the kernels that take the panel otherwise: DESIGN 3.9.
// A narrow call whose rows average less than three quarters of the bar does not classify at all: the classifier,
// an LDS-tiled launch that every workgroup leaves at once and the per-row ownership test of the direct kernel cost a
// 1 M-row matrix of 5 nonzeros per row 0.23 ms of a 0.09 ms product (N = 8).
static float window_min_rowlen(int64_t ldbt)
{
    const int t = options().rowlen_bar;
    if (t > 1) return (float)t; /* SBLAS_TUNE=*,<nonzeros per row>: threshold sweeps */
    // 64+ columns, banded rows, 1 M rows, LDS-tiled kernel | four rows per wave (ms): N = 64: 5 per row .737 | .565, 16: .796 | .669,
    // 24: .849 | .804, 32: .924 | .944, 48: 1.06 | 1.22; N = 256: 16: 3.01 | 2.65, 24: 3.17 | 3.20, 32: 3.41 | 3.76
    if (ldbt >= 64) return 24.0f;
    // banded rows, 1 M rows, LDS-tiled kernel | lane groups (ms): N = 8: 27 per row .418 | .283, 40: .464 | .377, 60: .524 | .547,
    // 80: .466 | .554; N = 16: 10: .452 | .287, 27: .483 | .540; N = 32: 10: .672 | .553, 27: .711 | 1.04
    return ldbt <= 8 ? 56.0f : ldbt <= 16 ? 20.0f : 16.0f;
}
// what the classifier looks at for the direct kernels' sake (128+ staged columns): bit 0 rows that share column patterns
// (row-merging kernel), bit 1 column runs / row-length spread (row per wave or four rows per wave)
static int direct_probe(int64_t ldbt) { return ldbt >= 128 ? (options().direct_merge ? 3 : 2) : 0; }
static bool classify_worthwhile(int64_t rows, int64_t nnz, int64_t ldbt)
{
    // (128+ staged columns: the classifier also feeds the matrix-core and row-merging choices; a forced matrix-core run
    //  needs its verdicts at any width)
    return ldbt >= 128 || (ldbt >= 64 && options().spmm_variant == SPMM_VARIANT_MFMA) || (rows > 0 && (double)nnz >= 0.75 * (double)window_min_rowlen(ldbt) * (double)rows);
}
// block fill from which a panel goes to the matrix cores (fp64 MFMA and fp64 vector FMA have the same peak on gfx950,
// so the zero fill of a block is paid in full): measured break-even against the vector kernels, tools/spmm_shapes.py blocks:ROWS:FILL
static float mfma_min_fill(int variant, int panel_rows, int64_t ldbt)
{
    if (panel_rows > 16 * MFMA_MAX_WAVES) return 2.0f; // the matrix-core kernel runs one wave per 16 rows of a panel
    if (variant == SPMM_VARIANT_MFMA) return 0.0f;
    if (variant == SPMM_VARIANT_NO_MFMA) return 2.0f;
    // Measured (tools/spmm_shapes.py): a chunk step of the matrix-core kernel costs ~2600 cycles of
    // instruction issue whatever the width, so it needs 128+ dense columns (8+ MFMAs per block) to pay: block-
    // structured rows at 60 % fill, N = 128: 0.57 ms against 0.65 ms for the LDS-tiled kernel; N = 64: 0.40 against
    // 0.31 ms; N = 256 at 35 % fill: 1.55 against 1.29 ms; grid-structured Queen-like rows (fill 0.32), N = 256: 2.33
    // against 2.16 ms for the direct kernel.  64-column calls therefore never take it unless SBLAS_MFMA_MIN_FILL says so.
    const float f = options().mfma_min_fill;
    if (f >= 0.0f) return f;
    return ldbt >= 128 ? 0.5f : 2.0f;
}
ClassifyArgs classify_args(int panel_rows, int64_t ldbt)
{
    return {1 << 24, window_min_density(panel_rows), window_min_rowlen(ldbt),
            ldbt < 64 ? 2.0f : mfma_min_fill(options().spmm_variant, panel_rows, ldbt), direct_probe(ldbt)};
}

// ---------------------------------------------------------------------------------------------
// What a column chunk of an SpMM call does before stage 2, decided once (spmm_step) and carried out by launch_stage and
// launch_spmm_rowpanel.  A plan (sblas_hip_spmm_plan_create) keeps the verdicts of the decision it asked for here.
// ---------------------------------------------------------------------------------------------
// SBLAS_SPMM_VARIANT: "dpp" and "rows" pin a direct kernel at every width, "merge" at 64+ staged columns (where the
// row-merging kernel exists) and "lanes" at narrow ones (the lane-group kernel): no panel is classified there
static bool variant_classifies(int v, int64_t ldbt)
{
    return v != SPMM_VARIANT_DIRECT_DPP && v != SPMM_VARIANT_DIRECT_ROWS &&
           v != (ldbt >= 64 ? SPMM_VARIANT_DIRECT_MERGE : SPMM_VARIANT_LANES);
}
// ... and only the variants that pin no kernel at any width take a plan
static bool variant_plannable(int v)
{
    return v == SPMM_VARIANT_AUTO || v == SPMM_VARIANT_MFMA || v == SPMM_VARIANT_NO_MFMA;
}
// a staging copy of ldbt columns beyond the 32-bit byte offsets the 16- / 32-column direct kernel addresses Bt with
static bool bt_beyond_32bit(int64_t cols, int64_t ldbt) { return ((uint64_t)cols + 1) * (uint64_t)ldbt * 8ull > 0xffffffffull; }
// Staging traffic saved if a row block's columns span no more than twice its rows, against the extra pass over the column
// indices and one more launch (~5 us = 40 MB at staging speed; a quarter of nd24k at N = 128 breaks even, an eighth of a
// Queen-like matrix at N = 256 runs 1.5x faster: tools/spmm_shapes.py --block)
static bool range_staging_pays(int64_t rows, int64_t cols, int64_t nnz, int64_t ldbt)
{
    return cols > 2 * rows && (uint64_t)(cols - 2 * rows) * (uint64_t)ldbt * 16ull > (uint64_t)nnz * 8ull + (40ull << 20);
}
int range_parts(int64_t nnz) { return (int)std::max<int64_t>(1, std::min<int64_t>((nnz + 4095) / 4096, TAIL_PARTS)); }

// spmm_step without its epoch (`again`: the previous chunk's verdicts, and so its epoch, still stand).  ncu: compute
// units of the device, 0 = ask for them (compute_units) should the panel height be needed
static SpmmStep step_rule(int rows, int cols, int64_t nnz, int64_t ldbt, const PlanView *pv, const SpmmStep &prev,
                          bool caller_staged, int ncu, bool &again)
{
    SpmmStep st;
    st.ldbt = ldbt;
    st.pv = pv;
    again = false;
    if (pv) { // classified, voted on and counted once: only B is left to stage
        st.staging = STAGE_PLANNED, st.verdicts = VERDICTS_PLAN;
        st.info_rows = pv->info_rows, st.groups = pv->groups;
        st.npanels = (int)(((int64_t)rows + st.info_rows - 1) / st.info_rows);
        return st;
    }
    const Options &opt = options();
    const bool classify = variant_classifies(opt.spmm_variant, ldbt) && (ldbt >= 64 || !bt_beyond_32bit(cols, ldbt)) &&
                          classify_worthwhile(rows, nnz, ldbt);
    // a row block (method 2): the row-major copy covers only the rows of B the block's nonzeros refer to
    const bool range = !caller_staged && ldbt >= 64 &&
                       (opt.stage_range > 0 || (opt.stage_range < 0 && range_staging_pays(rows, cols, nnz, ldbt)));
    // the classifier rides in the staging launch (one launch and one gap less per call) wherever there is one
    st.staging = caller_staged ? STAGE_CALLER : range ? STAGE_RANGE : classify ? STAGE_FUSED : STAGE_FULL;
    st.plannable = classify && !caller_staged && variant_plannable(opt.spmm_variant);
    if (classify) {
        panel_plan(rows, ldbt, ncu > 0 ? ncu : compute_units(), st.info_rows, st.groups);
        st.npanels = (int)(((int64_t)rows + st.info_rows - 1) / st.info_rows);
    }
    // a later column chunk of a range-staged call (same A, same ldbt, same workspace): the column range and the panel
    // verdicts in the tail still stand, only B's next columns need staging
    again = classify && range && prev.staging == STAGE_RANGE && prev.verdicts != VERDICTS_NONE && prev.ldbt == ldbt;
    st.verdicts = !classify ? VERDICTS_NONE : again ? VERDICTS_EARLIER : caller_staged ? VERDICTS_SEPARATE : VERDICTS_STAGING;
    return st;
}

SpmmStep spmm_step(int rows, int cols, int64_t nnz, int64_t ldbt, const PlanView *pv, const SpmmStep &prev, bool caller_staged)
{
    bool again = false;
    SpmmStep st = step_rule(rows, cols, nnz, ldbt, pv, prev, caller_staged, 0, again);
    st.epoch = pv ? pv->epoch : again ? prev.epoch : next_epoch();
    return st;
}

// ---------------------------------------------------------------------------------------------
// Stage 2 of a chunk: 1. the LDS-tiled kernel and 2. the matrix-core kernel on the panels that qualify, 3. a direct kernel
// on the rest -- on everything when nothing is classified.  A planned call launches only the kernels that have panels.
// ---------------------------------------------------------------------------------------------
SpmmStage2 spmm_stage2(const SpmmStep &st, int rows, int cols, int64_t nnz, int n)
{
    SpmmStage2 d;
    const Options &opt = options();
    const int variant = opt.spmm_variant;
    const int64_t ldbt = st.ldbt;
    const PlanView *pv = st.pv;
    const double avg_row = rows > 0 ? (double)nnz / (double)rows : 0.0;
    const bool classified = st.verdicts != VERDICTS_NONE;
    const bool need_window = !pv || pv->n_window + pv->n_mfma_w > 0;
    const bool need_mfma = !pv || pv->n_mfma_w + pv->n_mfma_d > 0;
    const bool need_direct = !pv || pv->n_direct + pv->n_mfma_d > 0;
    d.g = st.groups;
    d.interleave = opt.direct_map;
    d.dpp_long = opt.dpp_long;
    // a split plan: the direct kernels leave the split rows alone, the split kernels follow them
    d.skip = pv && pv->n_split > 0;
    d.split_groups = ldbt >= 128 ? 1 : ldbt == 64 ? 2 : 4;
    // the four-rows-per-wave direct kernel.  Workgroups of 4 waves (16 rows) for the shortest rows, 16 waves (64 rows) otherwise:
    // 1 M banded rows of 5 / 10 / 20 / 32 per row, N = 64, 4 | 8 | 16 waves: 0.547 | 0.554 | 0.571, 0.632 | 0.613 | 0.617, 0.973 |
    // 0.936 | 0.912, 1.22 | 1.17 | 1.14 ms; power-law rows averaging 3.2 (a 64-row workgroup waits for its longest row): 0.740 |
    // 0.830 | 0.957 ms.  (SBLAS_TUNE=*,*,*,<4|8|16> pins the size: A/B runs)
    d.rows_waves = opt.rows_waves ? opt.rows_waves : avg_row < 8.0 ? 4 : 16;
    if (ldbt >= 64) {
        if (classified) {
            // 128+ staged columns: two 64-column halves per workgroup, the selection work of a (rows, tile) visit shared
            // (SBLAS_TUNE=*,1 keeps one half per workgroup: A/B runs)
            const bool two_halves = ldbt >= 128 && !opt.one_half;
            if (need_window) {
                d.tiled = TILED_WINDOW6;
                d.g = st.groups == 3 ? 3 : 2;
                d.nh = d.g == 2 && two_halves ? 2 : 1;
                d.grid_y = (int)(ldbt / (two_halves ? 128 : 64));
            }
            d.mfma = need_mfma && mfma_min_fill(variant, st.info_rows, ldbt) <= 1.0f;
            d.mfma_batch = ldbt == 64 ? opt.mfma_batch64 : opt.mfma_batch128;
            d.mfma_lds_floor = opt.mfma_lds_floor;
        }
        // 128-column tiles: one workgroup per CU through unused dynamic LDS (Queen-like rows at N = 256: +13 %, banded
        // matrix at N = 128: +3 %); SBLAS_DIRECT_LDS overrides (experiments: rows in flight vs L2 reach)
        d.dpp_pad = opt.direct_lds >= 0 ? (size_t)opt.direct_lds : (ldbt == 64 ? 0 : 90000);
        if (!need_direct) {
        } else if (n > 32 && (variant == SPMM_VARIANT_DIRECT_ROWS ||
                              (variant != SPMM_VARIANT_DIRECT_DPP && avg_row < (ldbt == 64 ? 56.0 : 32.0)))) {
            // short rows: four rows per wave (64 staged columns, banded rows, 1 M rows, against the lane-group kernel: 32 per
            // row 1.08 | 1.14 ms, 48: 1.41 | 1.54, 64: 1.75 | 1.70, 100: 2.57 | 2.49)
            d.four_rows = true;
        } else if (ldbt == 64) {
            d.dpp = n <= 32 ? 4 : 2;
        } else {
            // 128-column tiles.  Classified calls launch both direct kernels: the classifier's vote (device side) says
            // whether the rows share column patterns, and the kernel whose call it is not leaves on one scalar load.
            d.merge = pv ? pv->merge : variant == SPMM_VARIANT_DIRECT_MERGE || (classified && opt.direct_merge);
            d.dpp = (pv ? !pv->merge && !pv->four_rows : variant != SPMM_VARIANT_DIRECT_MERGE) ? 1 : 0;
            // ... and whether four rows per wave on 64-column tiles suit them better than a row per wave on 128-column tiles
            d.four_rows = pv ? pv->four_rows : classified && variant != SPMM_VARIANT_DIRECT_MERGE;
            d.voted = d.four_rows && !pv ? 1 : 0;
        }
        return d;
    }
    // ---- narrow dense blocks (ldbt = 8 / 16 / 32): LDS-tiled lane-per-entry kernel on the panels that qualify, a direct
    // kernel on the rest
    if (classified && need_window) {
        const int g = st.groups;
        d.tiled = TILED_LANES;
        d.nc = (int)ldbt;
        if (ldbt == 8) {
            d.cp = opt.lanes_copies, d.g = g == 3 ? 3 : g == 2 ? 2 : 1, d.lpe = 1;
        } else if (ldbt == 16) {
            // three groups: two lanes per entry (eight accumulators per lane and group)
            d.cp = opt.lanes_copies == 2 ? 2 : 1;
            d.g = g == 3 && d.cp == 1 ? 3 : g == 2 ? 2 : 1;
            d.lpe = d.g == 3 ? 2 : 1;
        } else {
            // 32 columns: two lanes per entry (sixteen accumulators per lane: two groups of rows per wave fit), or a
            // lane per entry with one group (SBLAS_TUNE=*,*,*,1: A/B runs)
            d.cp = 1, d.g = g == 2 ? 2 : 1;
            d.lpe = d.g == 1 && opt.lanes32_one_lane ? 1 : 2;
        }
    }
    // short rows leave most of a row-per-wave sweep empty: lane groups below 24 / 16 nonzeros per row on average at 16 / 32
    // columns (banded rows of 5 / 10 per row, 1 M rows: N = 16 0.214 / 0.287 ms against 0.585 / 0.667 row per wave; N = 32
    // 0.403 / 0.553 against 0.691 / 0.758; from 27 per row on the row-per-wave kernel wins)
    const bool short_rows = ldbt >= 16 && avg_row < (ldbt == 16 ? 24.0 : 16.0) && variant != SPMM_VARIANT_DIRECT_DPP;
    if (!need_direct) {
    } else if (ldbt >= 16 && !bt_beyond_32bit(cols, ldbt) && variant != SPMM_VARIANT_LANES && !short_rows) {
        // the row-per-wave kernel, four nonzeros per instruction: sixteen lanes x 16 bytes per nonzero (with 16 staged
        // columns the upper eight lanes of a DPP row read past the Bt row, into columns that are never stored); it
        // addresses Bt with 32-bit byte offsets
        d.dpp = 4;
    } else if (ldbt >= 16) {
        d.narrow = (int)ldbt;
    } else if (avg_row >= opt.rows8_min_avg && variant != SPMM_VARIANT_LANES) {
        // n <= 8, long rows: a wave per row, eight sums per lane (banded-random rows, band +-20000, 600 k rows,
        // N = 8: 64 / 128 / 200 / 300 per row: the lane groups win by 25 / 30 / 2 / 0 %; bench matrix, 399 per row,
        // band +-2000: the wave per row wins by 20 % -- tools/rows8_threshold.py)
        d.rows8 = true;
    } else {
        d.narrow = 8;
    }
    return d;
}

} // namespace sblas

extern "C" int64_t sblas_spmm_rule_describe(int64_t rows, int64_t cols, int64_t nnz, int64_t ldbt, int64_t n, int64_t ncu,
                                            int caller_staged, const int64_t *plan, int64_t *out, int64_t max_out)
{
    const bool width_ok = ldbt == 8 || ldbt == 16 || ldbt == 32 || ldbt == 64 || (ldbt >= 128 && ldbt % 128 == 0);
    if (rows < 0 || rows > INT32_MAX || cols < 0 || cols >= INT32_MAX || nnz < 0 || !width_ok || n < 1 || n > ldbt || ncu < 1 ||
        ncu > INT32_MAX || (out && max_out < 0))
        return -1;
    sblas::PlanView pv;
    if (plan) {
        for (int k = 0; k < SBLAS_SPMM_RULE_PLAN_FIELDS; ++k)
            if (plan[k] < 0) return -1;
        if (plan[SBLAS_SPMM_RULE_PLAN_PANEL_ROWS] < 1 || plan[SBLAS_SPMM_RULE_PLAN_PANEL_ROWS] > INT32_MAX ||
            plan[SBLAS_SPMM_RULE_PLAN_GROUPS] > INT32_MAX || caller_staged)
            return -1;
        pv.n_window = (long)plan[SBLAS_SPMM_RULE_PLAN_N_WINDOW], pv.n_direct = (long)plan[SBLAS_SPMM_RULE_PLAN_N_DIRECT];
        pv.n_mfma_w = (long)plan[SBLAS_SPMM_RULE_PLAN_N_MFMA_W], pv.n_mfma_d = (long)plan[SBLAS_SPMM_RULE_PLAN_N_MFMA_D];
        pv.merge = plan[SBLAS_SPMM_RULE_PLAN_MERGE] != 0, pv.four_rows = plan[SBLAS_SPMM_RULE_PLAN_FOUR_ROWS] != 0;
        pv.n_split = plan[SBLAS_SPMM_RULE_PLAN_N_SPLIT];
        pv.info_rows = (int)plan[SBLAS_SPMM_RULE_PLAN_PANEL_ROWS], pv.groups = (int)plan[SBLAS_SPMM_RULE_PLAN_GROUPS];
    }
    bool again = false;
    const sblas::SpmmStep st = sblas::step_rule((int)rows, (int)cols, nnz, ldbt, plan ? &pv : nullptr, sblas::SpmmStep(),
                                                caller_staged != 0, (int)ncu, again); // (no epoch is drawn)
    const sblas::SpmmStage2 d = sblas::spmm_stage2(st, (int)rows, (int)cols, nnz, (int)n);
    int64_t f[SBLAS_SPMM_RULE_FIELDS] = {0};
    f[SBLAS_SPMM_RULE_STAGING] = st.staging, f[SBLAS_SPMM_RULE_VERDICTS] = st.verdicts;
    f[SBLAS_SPMM_RULE_PANEL_ROWS] = st.info_rows, f[SBLAS_SPMM_RULE_GROUPS] = st.groups;
    f[SBLAS_SPMM_RULE_PANELS] = st.npanels, f[SBLAS_SPMM_RULE_PLANNABLE] = st.plannable;
    f[SBLAS_SPMM_RULE_TILED] = d.tiled, f[SBLAS_SPMM_RULE_TILED_G] = d.tiled ? d.g : 0;
    f[SBLAS_SPMM_RULE_W6_NH] = d.nh, f[SBLAS_SPMM_RULE_W6_GRID_Y] = d.grid_y;
    f[SBLAS_SPMM_RULE_LANES_NC] = d.nc, f[SBLAS_SPMM_RULE_LANES_CP] = d.cp, f[SBLAS_SPMM_RULE_LANES_LPE] = d.lpe;
    f[SBLAS_SPMM_RULE_MFMA] = d.mfma;
    f[SBLAS_SPMM_RULE_MFMA_BATCH] = d.mfma ? d.mfma_batch : 0;
    f[SBLAS_SPMM_RULE_MFMA_LDS_FLOOR] = d.mfma ? (int64_t)d.mfma_lds_floor : 0;
    f[SBLAS_SPMM_RULE_FOUR_ROWS] = d.four_rows;
    f[SBLAS_SPMM_RULE_FOUR_ROWS_WAVES] = d.four_rows ? d.rows_waves : 0;
    f[SBLAS_SPMM_RULE_FOUR_ROWS_VOTED] = d.voted;
    f[SBLAS_SPMM_RULE_MERGE] = d.merge;
    f[SBLAS_SPMM_RULE_DPP_GROUPS] = d.dpp;
    f[SBLAS_SPMM_RULE_DPP_PAD] = d.dpp ? (int64_t)d.dpp_pad : 0;
    f[SBLAS_SPMM_RULE_DPP_LONG] = d.dpp ? d.dpp_long : 0;
    f[SBLAS_SPMM_RULE_NARROW] = d.narrow, f[SBLAS_SPMM_RULE_ROWS8] = d.rows8;
    f[SBLAS_SPMM_RULE_INTERLEAVE] = d.interleave;
    f[SBLAS_SPMM_RULE_SKIP] = d.skip, f[SBLAS_SPMM_RULE_SPLIT_GROUPS] = d.skip ? d.split_groups : 0;
    for (int64_t k = 0; out && k < SBLAS_SPMM_RULE_FIELDS && k < max_out; ++k) out[k] = f[k];
    return SBLAS_SPMM_RULE_FIELDS;
}
