// capi.hip -- the extern "C" surface declared in include/sblas_hip.h (compute entry points).
// Argument checking happens here, on the host, before any kernel is launched: a bad shape, leading dimension, pointer or
// workspace comes back as SBLAS_E_INVALID / SBLAS_E_WORKSPACE.  The CONTENTS of the index arrays are the caller's
// contract, as with the vendor libraries this replaces (a column index outside [0, cols) is an out-of-bounds read);
// SBLAS_VALIDATE=1 / sblas_hip_debug_validate_csr_i32 check them on the device first, at the price of a synchronisation.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <memory>
#include <vector>
#include "../../include/sblas_hip.h"
#include "capi_util.h"
#include "kernels.h"

extern "C" {

int sblas_hip_version(void) { return 100; }

const char *sblas_hip_error_string(int code)
{
    switch (code) {
    case SBLAS_OK: return "success";
    case SBLAS_E_INVALID: return "invalid argument";
    case SBLAS_E_HIP: return "HIP runtime / kernel launch failure";
    case SBLAS_E_WORKSPACE: return "workspace missing or too small";
    case SBLAS_E_RCCL: return "RCCL unavailable or collective failed";
    case SBLAS_E_IO: return "MatrixMarket read/parse failure";
    case SBLAS_E_NOGPU: return "no HIP device";
    case SBLAS_E_INTERNAL: return "internal error (a device loop made no progress)";
    default: return "unknown sblas error";
    }
}

int sblas_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// staged width of an n-column block: 8, 16 (tier16), 32 (tier32), 64 or a multiple of 128.  The 16- / 32-column tiers are
// also the last resort when even a 64-column staging copy would exceed the 32-bit offset window (chunk_ldbt).
static int64_t ldbt_pick(int64_t n, bool tier16, bool tier32)
{
    if (n <= 0) return 0;
    if (n <= 8) return 8;
    if (n <= 16 && tier16) return 16;
    if (n <= 32 && tier32) return 32;
    if (n <= 64) return 64;
    return (n + 127) / 128 * 128; // wide tiles are 128 columns (two per lane)
}

int64_t sblas_hip_spmm_ldbt(int64_t n)
{
    // 8 / 16 / 32 / 64 staged columns for n <= 8 / 16 / 32 / 64: method 1 on 8 / 4 / 2 GPUs hands a GPU exactly these
    // widths of a 64-column B (matrix.h:554-568), and the narrow LDS-tiled kernel (spmm_lanes_kernel) reads NC * 8 bytes
    // of LDS per nonzero instead of the 512 of a zero-padded 64-column tile (banded bench matrix, N = 8 / 16 / 32 on the
    // 64-column path: 0.265 / 0.238 / 0.245 ms).  SBLAS_SPMM_MIN_LDBT=64 puts 9..32 columns back on the 64-column
    // staging copy (A/B runs, tests).
    return ldbt_pick(n, sblas::options().tier16, sblas::options().tier32);
}
static bool ldbt_ok(int64_t ldbt, int64_t n)
{
    return ldbt == ldbt_pick(n, false, false) || ldbt == ldbt_pick(n, true, true) || ldbt == ldbt_pick(n, true, false) ||
           ldbt == ldbt_pick(n, false, true);
}

// The kernels address Bt with 32-bit byte offsets, so one stage-2 launch can cover at most 4 GiB of Bt.  The
// top-level call therefore walks the dense columns in chunks of `w` columns with (cols+1)*ldbt(w)*8 <= 4 GiB
// (Queen_4147 with N = 256: two chunks of 128).  SBLAS_SPMM_MAX_BT_BYTES lowers the limit (tests).
static uint64_t bt_byte_limit() { return sblas::options().max_bt_bytes; }

static int64_t spmm_chunk_cols(int64_t cols, int64_t n)
{
    const uint64_t lim = bt_byte_limit();
    const uint64_t row_bytes = 8ull * ((uint64_t)cols + 1);
    if (row_bytes * (uint64_t)sblas_hip_spmm_ldbt(n) <= lim) return n;
    for (int64_t w = (n / 128) * 128; w >= 128; w -= 128)
        if (row_bytes * (uint64_t)w <= lim) return w;
    if (row_bytes * 64ull <= lim) return 64;
    return 32; // the narrow kernels use 64-bit addressing: no limit
}
// ldbt of a chunk of nj columns: the narrow tier when the chunk width itself was forced down to 32
static int64_t chunk_ldbt(int64_t cols, int64_t n, int64_t nj)
{
    const bool forced_narrow = spmm_chunk_cols(cols, n) <= 32 && 8ull * ((uint64_t)cols + 1) * 64ull > bt_byte_limit();
    return forced_narrow ? ldbt_pick(nj, true, true) : sblas_hip_spmm_ldbt(nj);
}

size_t sblas_hip_spmm_csr_f64_i32_workspace(int64_t rows, int64_t cols, int64_t nnz, int64_t n)
{
    (void)nnz;
    if (cols <= 0 || n <= 0) return 0;
    // Bt for one column chunk plus one extra all-zero row (the target of masked DPP slots), then one int2 per
    // row panel (the panel classifier's verdicts)
    const int64_t w = spmm_chunk_cols(cols, n);
    const size_t bt = ((size_t)cols + 1) * (size_t)chunk_ldbt(cols, n, w) * sizeof(double);
    return bt + sblas::workspace_tail_bytes(rows); // flags, one span and one class per row panel
}

int sblas_hip_dense_to_rowmajor_f64(int dev, void *stream, int64_t cols, int64_t n, const double *B,
                                    int64_t ldb, double *Bt, int64_t ldbt)
{
    if (cols < 0 || n < 0) return SBLAS_E_INVALID;
    if (cols == 0 || n == 0) return SBLAS_OK;
    if (!B || !Bt || ldb < cols || ldbt < n || !ldbt_ok(ldbt, n)) return SBLAS_E_INVALID;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    return sblas::launch_dense_to_rowmajor((hipStream_t)stream, cols, n, B, ldb, Bt, ldbt, false) == hipSuccess ? SBLAS_OK
                                                                                                             : SBLAS_E_HIP;
}

// A has no nonzeros (cols == 0 or nnz == 0): C = beta * C, nothing else.  Neither the staging copy nor the panel
// verdicts behind it are touched, so a NULL / empty workspace is fine here.
static int scale_only(int dev, void *stream, int64_t rows, int64_t n, double beta, double *C, int64_t ldc, int order_c)
{
    if (beta == 1.0) return SBLAS_OK;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    return sblas::launch_scale((hipStream_t)stream, rows, n, beta, C, ldc, order_c == SBLAS_ROW_MAJOR) == hipSuccess
               ? SBLAS_OK
               : SBLAS_E_HIP;
}

int sblas_hip_spmm_csr_rowmajorB_f64_i32(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz,
                                         const int32_t *rowptr, const int32_t *colidx, const double *val,
                                         const double *Bt, int64_t ldbt, int64_t n, double alpha,
                                         double beta, double *C, int64_t ldc)
{
    if (!csr_args_ok(rows, cols, nnz, rowptr, colidx, val) || n < 0) return SBLAS_E_INVALID;
    if (rows == 0 || n == 0) return SBLAS_OK;
    if (!C || ldc < rows || n > INT_MAX) return SBLAS_E_INVALID;
    if (!ldbt_ok(ldbt, n)) return SBLAS_E_INVALID;
    if (cols == 0 || nnz == 0) return scale_only(dev, stream, rows, n, beta, C, ldc, SBLAS_COL_MAJOR); // A*B = 0: no kernel reads Bt
    if (!Bt || !aligned16(Bt)) return SBLAS_E_INVALID;
    // the kernels address Bt with 32-bit element offsets (row * ldbt + column)
    if (ldbt >= 64 && ((uint64_t)cols + 1) * (uint64_t)ldbt * 8ull > 0xffffffffull) return SBLAS_E_INVALID; // 32-bit byte offsets
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    const sblas::SpmmStep st = sblas::spmm_step((int)rows, (int)cols, nnz, ldbt, nullptr, sblas::SpmmStep(), true);
    return sblas::launch_spmm_rowpanel((hipStream_t)stream, st, (int)rows, (int)cols, nnz, rowptr, colidx, val, Bt, (int)n,
                                       alpha, beta, C, ldc, false) == hipSuccess
               ? SBLAS_OK
               : SBLAS_E_HIP;
}

static int validate_if_asked(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr,
                             const int32_t *colidx);

namespace {

// What a plan speaks for: ONE structure -- the same arrays it was made from (their contents are the caller's promise) --
// on the device its buffers live on.  A planned call for anything else is refused.
struct PlanKey {
    int dev = -1;
    int64_t rows = 0, cols = 0, nnz = 0;
    const void *rowptr = nullptr, *colidx = nullptr;
    bool speaks_for(int dev_arg, int64_t r, int64_t c, int64_t z, const void *rp, const void *ci) const
    {
        return dev == resolve_device(dev_arg) && rows == r && cols == c && nnz == z && rowptr == rp && colidx == ci;
    }
};

// A plan: the panel verdicts of one matrix structure at one staged width, taken once (sblas_hip_spmm_plan_create).
struct SpmmPlan : PlanKey {
    int64_t n = 0, ldbt = 0;
    bool active = false;        // false: nothing to plan (empty matrix, a pinned direct variant): calls run unplanned
    DeviceBuffer buf;
    DeviceBuffer split_buf;     // a split plan's partial sums, row bitmap, pieces and split rows
    sblas::PlanView pv;
};

// A per-matrix SpMV plan (sblas_hip_spmv_plan_create).  One device buffer: the partial sums of the split pieces (doubles)
// first, then the int4 work items of the kernel classes, the pieces and the split rows.
struct SpmvPlan : PlanKey {
    bool active = false; // false: empty matrix or a pinned SBLAS_SPMV_VARIANT: calls run unplanned
    DeviceBuffer buf;
    sblas::SpmvPlanView pv;
};

} // namespace

// The <f64, i32> SpMM of every entry point.  B and C each column- or row-major (order_b / order_c): B's layout reaches
// only the staging launch, C's only the stage-2 epilogues; Bt, the workspace and the plan are the same for all four.
static int spmm_impl(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr,
                     const int32_t *colidx, const double *val, const double *B, int64_t ldb, int order_b, int64_t n,
                     double alpha, double beta, double *C, int64_t ldc, int order_c, void *workspace,
                     size_t workspace_bytes, const SpmmPlan *plan)
{
    if (!order_ok(order_b) || !order_ok(order_c)) return SBLAS_E_INVALID;
    if (!csr_args_ok(rows, cols, nnz, rowptr, colidx, val) || n < 0) return SBLAS_E_INVALID;
    if (rows == 0 || n == 0) return SBLAS_OK;
    if (!C || !ld_ok(order_c, ldc, rows, n)) return SBLAS_E_INVALID;
    if (cols > 0 && (!B || !ld_ok(order_b, ldb, cols, n))) return SBLAS_E_INVALID;
    if (cols == 0 || nnz == 0) return scale_only(dev, stream, rows, n, beta, C, ldc, order_c);
    if (const int vrc = validate_if_asked(dev, stream, rows, cols, nnz, rowptr, colidx)) return vrc;
    if (!workspace || workspace_bytes < sblas_hip_spmm_csr_f64_i32_workspace(rows, cols, nnz, n)) return SBLAS_E_WORKSPACE;
    if (!aligned16(workspace)) return SBLAS_E_INVALID;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    const hipStream_t s = (hipStream_t)stream;
    const bool row_b = order_b == SBLAS_ROW_MAJOR, row_c = order_c == SBLAS_ROW_MAJOR;
    double *Bt = static_cast<double *>(workspace);
    const int64_t w = spmm_chunk_cols(cols, n);
    sblas::SpmmStep step; // the previous chunk's
    for (int64_t j0 = 0; j0 < n; j0 += w) { // one pass unless Bt would exceed the 32-bit offset window
        const int64_t nj = (n - j0 < w) ? n - j0 : w;
        const int64_t ldbt = chunk_ldbt(cols, n, nj);
        const sblas::PlanView *pv = plan && plan->active && ldbt == plan->ldbt ? &plan->pv : nullptr;
        step = sblas::spmm_step((int)rows, (int)cols, nnz, ldbt, pv, step);
        if (sblas::launch_stage(s, step, (int)rows, cols, nnz, rowptr, colidx, nj, col_at(B, order_b, ldb, j0), ldb, Bt, row_b) !=
                hipSuccess ||
            sblas::launch_spmm_rowpanel(s, step, (int)rows, (int)cols, nnz, rowptr, colidx, val, Bt, (int)nj, alpha, beta,
                                        col_at(C, order_c, ldc, j0), ldc, row_c) != hipSuccess)
            return SBLAS_E_HIP;
    }
    return SBLAS_OK;
}

int sblas_hip_spmm_csr_f64_i32(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz,
                               const int32_t *rowptr, const int32_t *colidx, const double *val,
                               const double *B, int64_t ldb, int64_t n, double alpha, double beta,
                               double *C, int64_t ldc, void *workspace, size_t workspace_bytes)
{
    return spmm_impl(dev, stream, rows, cols, nnz, rowptr, colidx, val, B, ldb, SBLAS_COL_MAJOR, n, alpha, beta, C, ldc,
                     SBLAS_COL_MAJOR, workspace, workspace_bytes, nullptr);
}

// ---- per-matrix plan (the slot of cusparseSpMM_bufferSize / preprocess, spmm.h:134-141) --------------------------

// A split plan's long rows (sblas_hip_spmm_plan_create_split): the classifier on host copies of rowptr and the panel
// verdicts, then one device buffer -- partial sums, row bitmap, pieces, split rows.
static hipError_t spmm_plan_split(SpmmPlan *p, hipStream_t s, const int32_t *rowptr, const std::vector<int> &cls,
                                  int64_t split_min, int64_t piece, bool *bad_rowptr)
{
    sblas::PlanView &pv = p->pv;
    const int64_t rows = p->rows;
    std::vector<int32_t> rp((size_t)rows + 1);
    hipError_t e = hipMemcpyAsync(rp.data(), rowptr, rp.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    // the panels the direct kernels own; none when the row-merging kernel takes them
    std::vector<uint8_t> mask(cls.size());
    for (size_t q = 0; q < cls.size(); ++q) mask[q] = !pv.merge && (cls[q] & sblas::PANEL_CLASS_MASK) == sblas::PANEL_DIRECT;
    const int64_t n_rec = sblas_spmm_split_classify(rp.data(), rows, p->nnz, split_min, piece, mask.data(), pv.info_rows, nullptr, 0);
    if (n_rec < 0) {
        *bad_rowptr = true;
        return hipSuccess;
    }
    if (n_rec == 0) return hipSuccess; // nothing to split: the plain plan
    std::vector<int4> rec((size_t)n_rec);
    if (sblas_spmm_split_classify(rp.data(), rows, p->nnz, split_min, piece, mask.data(), pv.info_rows,
                                  reinterpret_cast<int32_t *>(rec.data()), n_rec) != n_rec) {
        *bad_rowptr = true;
        return hipSuccess;
    }
    int64_t n_pieces = 0;
    while (n_pieces < n_rec && rec[(size_t)n_pieces].w >= 0) ++n_pieces;
    const int64_t n_split = n_rec - n_pieces;
    const size_t words = ((size_t)rows + 31) / 32;
    std::vector<unsigned> bits(words, 0u);
    int64_t split_nnz = 0;
    for (int64_t i = n_pieces; i < n_rec; ++i) {
        const int r = rec[(size_t)i].x;
        bits[(size_t)r / 32] |= 1u << (r % 32);
        split_nnz += (int64_t)rp[(size_t)r + 1] - rp[(size_t)r];
    }
    const size_t partial_bytes = (size_t)n_pieces * (size_t)p->ldbt * sizeof(double);
    const size_t bits_bytes = (words * sizeof(unsigned) + 15) / 16 * 16;
    if ((e = p->split_buf.alloc(p->dev, partial_bytes + bits_bytes + (size_t)n_rec * sizeof(int4))) != hipSuccess) return e;
    pv.partial = p->split_buf.at<double>();
    pv.split_bits = p->split_buf.at<const unsigned>(partial_bytes);
    pv.pieces = p->split_buf.at<const int4>(partial_bytes + bits_bytes);
    pv.srows = pv.pieces + n_pieces;
    if ((e = hipMemcpyAsync(p->split_buf.at<void>(partial_bytes), bits.data(), words * sizeof(unsigned), hipMemcpyHostToDevice,
                            s)) != hipSuccess)
        return e;
    if ((e = hipMemcpyAsync(p->split_buf.at<void>(partial_bytes + bits_bytes), rec.data(), (size_t)n_rec * sizeof(int4),
                            hipMemcpyHostToDevice, s)) != hipSuccess)
        return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e; // (the host images go next)
    pv.n_pieces = n_pieces, pv.n_split = n_split, pv.split_nnz = split_nnz;
    return hipSuccess;
}

static int spmm_plan_create(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr,
                            const int32_t *colidx, int64_t n, bool split, int64_t split_min, int64_t piece, void **plan_out)
{
    if (!plan_out || !csr_args_ok(rows, cols, nnz, rowptr, colidx, reinterpret_cast<const void *>(1)) || n < 0) return SBLAS_E_INVALID;
    *plan_out = nullptr;
    std::unique_ptr<SpmmPlan> p(new SpmmPlan);
    p->dev = resolve_device(dev), p->rows = rows, p->cols = cols, p->nnz = nnz, p->n = n, p->rowptr = rowptr, p->colidx = colidx;
    if (rows == 0 || cols == 0 || nnz == 0 || n == 0) { // nothing to plan
        *plan_out = p.release();
        return SBLAS_OK;
    }
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    // the step of the first column chunk; where it classifies nothing (a pinned direct kernel, short rows, a narrow Bt
    // beyond 32-bit offsets) the calls run unplanned
    const int64_t w = spmm_chunk_cols(cols, n);
    const int64_t ldbt = chunk_ldbt(cols, n, n < w ? n : w);
    const sblas::SpmmStep st = sblas::spmm_step((int)rows, (int)cols, nnz, ldbt, nullptr);
    if (st.plannable) {
        if (p->buf.alloc(p->dev, sblas::plan_tail_bytes(rows)) != hipSuccess) return SBLAS_E_HIP;
        p->pv.tail = p->buf.at<int>();
        p->ldbt = ldbt;
        std::vector<int> cls;
        if (sblas::plan_build((hipStream_t)stream, st, (int)rows, (int)cols, nnz, rowptr, colidx, &p->pv, split ? &cls : nullptr) !=
            hipSuccess)
            return SBLAS_E_HIP;
        if (split) {
            bool bad = false;
            if (spmm_plan_split(p.get(), (hipStream_t)stream, rowptr, cls, split_min, piece, &bad) != hipSuccess) return SBLAS_E_HIP;
            if (bad) return SBLAS_E_INVALID; // row pointers descending or outside [0, nnz]
        }
        p->active = true;
    }
    *plan_out = p.release();
    return SBLAS_OK;
}

int sblas_hip_spmm_plan_create(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr,
                               const int32_t *colidx, int64_t n, void **plan_out)
{
    return spmm_plan_create(dev, stream, rows, cols, nnz, rowptr, colidx, n, false, 0, 0, plan_out);
}

int sblas_hip_spmm_plan_create_split(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr,
                                     const int32_t *colidx, int64_t n, int64_t split_min, int64_t piece, void **plan_out)
{
    return spmm_plan_create(dev, stream, rows, cols, nnz, rowptr, colidx, n, true, split_min, piece, plan_out);
}

int sblas_hip_spmm_plan_destroy(void *plan)
{
    delete static_cast<SpmmPlan *>(plan);
    return SBLAS_OK;
}

int sblas_hip_spmm_plan_split_info(const void *plan, int64_t out[4])
{
    if (!plan || !out) return SBLAS_E_INVALID;
    const SpmmPlan *p = static_cast<const SpmmPlan *>(plan);
    out[0] = p->pv.n_split, out[1] = p->pv.n_pieces, out[2] = p->pv.split_nnz, out[3] = p->pv.n_pieces * p->ldbt * (int64_t)sizeof(double);
    return SBLAS_OK;
}

int sblas_hip_spmm_plan_info(const void *plan, int64_t out[8])
{
    if (!plan || !out) return SBLAS_E_INVALID;
    const SpmmPlan *p = static_cast<const SpmmPlan *>(plan);
    out[0] = p->active, out[1] = p->pv.n_window, out[2] = p->pv.n_direct, out[3] = p->pv.n_mfma_w + p->pv.n_mfma_d;
    out[4] = p->pv.merge ? 1 : p->pv.four_rows ? 2 : 0, out[5] = p->pv.use_range, out[6] = p->ldbt, out[7] = p->pv.info_rows;
    return SBLAS_OK;
}

int sblas_hip_spmm_csr_f64_i32_planned(const void *plan, int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz,
                                       const int32_t *rowptr, const int32_t *colidx, const double *val, const double *B,
                                       int64_t ldb, int64_t n, double alpha, double beta, double *C, int64_t ldc,
                                       void *workspace, size_t workspace_bytes)
{
    return sblas_hip_spmm_csr_ordered_f64_i32_planned(plan, dev, stream, rows, cols, nnz, rowptr, colidx, val, B, ldb,
                                                      SBLAS_COL_MAJOR, n, alpha, beta, C, ldc, SBLAS_COL_MAJOR, workspace,
                                                      workspace_bytes);
}

int sblas_hip_spmm_csr_ordered_f64_i32_planned(const void *plan, int dev, void *stream, int64_t rows, int64_t cols,
                                               int64_t nnz, const int32_t *rowptr, const int32_t *colidx, const double *val,
                                               const double *B, int64_t ldb, int order_b, int64_t n, double alpha,
                                               double beta, double *C, int64_t ldc, int order_c, void *workspace,
                                               size_t workspace_bytes)
{
    if (!plan || !order_ok(order_b) || !order_ok(order_c)) return SBLAS_E_INVALID;
    const SpmmPlan *p = static_cast<const SpmmPlan *>(plan);
    if (!p->speaks_for(dev, rows, cols, nnz, rowptr, colidx)) return SBLAS_E_INVALID;
    return spmm_impl(dev, stream, rows, cols, nnz, rowptr, colidx, val, B, ldb, order_b, n, alpha, beta, C, ldc, order_c,
                     workspace, workspace_bytes, p);
}

int sblas_hip_debug_validate_csr_i32(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr,
                                     const int32_t *colidx)
{
    if (!csr_args_ok(rows, cols, nnz, rowptr, colidx, reinterpret_cast<const void *>(1))) return SBLAS_E_INVALID;
    if (rows == 0) return SBLAS_OK;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    int bad = 0;
    if (sblas::validate_csr((hipStream_t)stream, rows, cols, nnz, rowptr, colidx, &bad) != hipSuccess) return SBLAS_E_HIP;
    return bad ? SBLAS_E_INVALID : SBLAS_OK;
}
static int validate_if_asked(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr,
                             const int32_t *colidx)
{
    if (!sblas::options().validate || rows <= 0 || nnz <= 0) return SBLAS_OK;
    return sblas_hip_debug_validate_csr_i32(dev, stream, rows, cols, nnz, rowptr, colidx);
}

int sblas_hip_debug_reload_env(void)
{
    sblas::options_reload();
    return SBLAS_OK;
}

int sblas_hip_debug_spmm_kernel_events(int enable)
{
    sblas::kernel_events_enable(enable != 0);
    return SBLAS_OK;
}

int sblas_hip_debug_spmm_last_kernel_ms(float *ms)
{
    if (!ms) return SBLAS_E_INVALID;
    return sblas::kernel_events_last_ms(ms) == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_debug_spmm_panel_stats(uint64_t out[4], int reset)
{
    if (!out) return SBLAS_E_INVALID;
    unsigned long long tmp[4];
    if (sblas::panel_stats(tmp, reset != 0) != hipSuccess) return SBLAS_E_HIP;
    for (int i = 0; i < 4; ++i) out[i] = tmp[i];
    return SBLAS_OK;
}

int sblas_hip_spmv_csr_f64_i32(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz,
                               const int32_t *rowptr, const int32_t *colidx, const double *val,
                               const double *x, double alpha, double beta, double *y)
{
    if (!csr_args_ok(rows, cols, nnz, rowptr, colidx, val)) return SBLAS_E_INVALID;
    if (rows == 0) return SBLAS_OK;
    if (!y || (cols > 0 && !x)) return SBLAS_E_INVALID;
    if (const int vrc = validate_if_asked(dev, stream, rows, cols, nnz, rowptr, colidx)) return vrc;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    return sblas::launch_spmv((hipStream_t)stream, (int)rows, (int)cols, nnz, rowptr, colidx, val, x, alpha, beta, y) ==
                   hipSuccess
               ? SBLAS_OK
               : SBLAS_E_HIP;
}

// ---- per-matrix SpMV plan (the slot of csrmv_analysis / cusparseSpMV_preprocess) --------------------------------
int sblas_hip_spmv_plan_create(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr,
                               const int32_t *colidx, void **plan_out)
{
    if (!plan_out || !csr_args_ok(rows, cols, nnz, rowptr, colidx, reinterpret_cast<const void *>(1))) return SBLAS_E_INVALID;
    *plan_out = nullptr;
    if (const int vrc = validate_if_asked(dev, stream, rows, cols, nnz, rowptr, colidx)) return vrc;
    std::unique_ptr<SpmvPlan> p(new SpmvPlan);
    p->dev = resolve_device(dev), p->rows = rows, p->cols = cols, p->nnz = nnz, p->rowptr = rowptr, p->colidx = colidx;
    if (rows == 0 || nnz == 0 || sblas::options().spmv_variant[0]) { // nothing to plan / a pinned kernel
        *plan_out = p.release();
        return SBLAS_OK;
    }
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int32_t> rp((size_t)rows + 1);
    if (hipMemcpyAsync(rp.data(), rowptr, rp.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return SBLAS_E_HIP;
    const int64_t n_items = sblas_spmv_plan_classify(rp.data(), rows, nnz, 0, 0, nullptr, 0);
    if (n_items <= 0 || rp[0] < 0 || rp[rows] > nnz) return SBLAS_E_INVALID; // row pointers descending or outside [0, nnz]
    std::vector<int4> it((size_t)n_items);
    if (sblas_spmv_plan_classify(rp.data(), rows, nnz, 0, 0, reinterpret_cast<int32_t *>(it.data()), n_items) != n_items)
        return SBLAS_E_INVALID;
    // host image of the buffer: items grouped by class (in row order inside a class), then pieces, then split rows
    sblas::SpmvPlanView &pv = p->pv;
    int64_t cnt[sblas::SPMV_ITEM_KERNELS] = {0};
    for (const int4 &q : it) {
        if (q.z == SBLAS_SPMV_ITEM_SPLIT) ++pv.n_split, pv.n_pieces += q.w;
        else ++cnt[q.z];
    }
    for (int k = 0; k < sblas::SPMV_ITEM_KERNELS; ++k) pv.off[k + 1] = pv.off[k] + cnt[k];
    const int64_t n_kernel_items = pv.off[sblas::SPMV_ITEM_KERNELS];
    std::vector<int4> img((size_t)(n_kernel_items + pv.n_pieces + pv.n_split));
    int64_t fill[sblas::SPMV_ITEM_KERNELS];
    for (int k = 0; k < sblas::SPMV_ITEM_KERNELS; ++k) fill[k] = pv.off[k];
    for (const int4 &q : it)
        if (q.z != SBLAS_SPMV_ITEM_SPLIT) img[fill[q.z]++] = make_int4(q.x, q.y, 0, -1);
    sblas::split_rows(rp.data(), rows, SBLAS_SPMV_SPLIT_PIECE, [](int64_t, int64_t len) { return len > SBLAS_SPMV_SPLIT_MIN; },
                      reinterpret_cast<int32_t *>(img.data() + n_kernel_items), pv.n_pieces + pv.n_split);
    const size_t partial_bytes = ((size_t)pv.n_pieces * sizeof(double) + 15) / 16 * 16;
    hipError_t e = p->buf.alloc(p->dev, partial_bytes + img.size() * sizeof(int4) + 16);
    if (e == hipSuccess) {
        pv.partial = p->buf.at<double>();
        pv.items = p->buf.at<int4>(partial_bytes);
        pv.pieces = pv.items + n_kernel_items;
        pv.srows = pv.pieces + pv.n_pieces;
        e = hipMemcpyAsync(pv.items, img.data(), img.size() * sizeof(int4), hipMemcpyHostToDevice, s);
    }
    if (e == hipSuccess)
        e = sblas::spmv_plan_windows(s, (int)(pv.off[SBLAS_SPMV_ITEM_LDS_S7 + 1] - pv.off[SBLAS_SPMV_ITEM_LDS_S2]),
                                     pv.items + pv.off[SBLAS_SPMV_ITEM_LDS_S2], rowptr, colidx);
    if (e == hipSuccess) e = hipStreamSynchronize(s); // (the host image is freed next)
    if (e != hipSuccess) return SBLAS_E_HIP;
    // one class, no split rows: the items are the unplanned kernel's own blocks (aligned from row 0, the launcher's
    // instantiation: both follow spmv_kind), so the unplanned launch computes the same thing without a load of the item at
    // every block's start (1 M banded rows of 7: 31.6 against 30.7 us).  The LDS-window class keeps its items: they carry
    // the column windows.
    int classes = 0;
    for (int k = 0; k < sblas::SPMV_ITEM_KERNELS; ++k) classes += pv.off[k + 1] > pv.off[k];
    pv.as_unplanned = classes == 1 && pv.n_split == 0 && pv.off[SBLAS_SPMV_ITEM_LDS_S2] == n_kernel_items;
    p->active = true;
    *plan_out = p.release();
    return SBLAS_OK;
}

int sblas_hip_spmv_plan_destroy(void *plan)
{
    delete static_cast<SpmvPlan *>(plan);
    return SBLAS_OK;
}

int sblas_hip_spmv_plan_speaks_for(const void *plan, int dev, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr,
                                   const int32_t *colidx)
{
    if (!plan) return SBLAS_E_INVALID;
    return static_cast<const SpmvPlan *>(plan)->speaks_for(dev, rows, cols, nnz, rowptr, colidx) ? SBLAS_OK : SBLAS_E_INVALID;
}

int sblas_hip_spmv_plan_info(const void *plan, int64_t out[8])
{
    if (!plan || !out) return SBLAS_E_INVALID;
    const SpmvPlan *p = static_cast<const SpmvPlan *>(plan);
    const int64_t *off = p->pv.off;
    auto n = [&](int k) { return off[k + 1] - off[k]; };
    out[0] = p->active;
    out[1] = n(SBLAS_SPMV_ITEM_LPR), out[2] = n(SBLAS_SPMV_ITEM_STREAM4096), out[3] = n(SBLAS_SPMV_ITEM_STREAM6144);
    out[4] = n(SBLAS_SPMV_ITEM_SEG), out[5] = off[SBLAS_SPMV_ITEM_LDS_S7 + 1] - off[SBLAS_SPMV_ITEM_LDS_S2];
    out[6] = p->pv.n_split, out[7] = p->pv.n_pieces;
    return SBLAS_OK;
}

int sblas_hip_spmv_csr_f64_i32_planned(const void *plan, int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz,
                                       const int32_t *rowptr, const int32_t *colidx, const double *val, const double *x,
                                       double alpha, double beta, double *y)
{
    if (!plan) return SBLAS_E_INVALID;
    const SpmvPlan *p = static_cast<const SpmvPlan *>(plan);
    if (!p->speaks_for(dev, rows, cols, nnz, rowptr, colidx)) return SBLAS_E_INVALID;
    if (!p->active) return sblas_hip_spmv_csr_f64_i32(dev, stream, rows, cols, nnz, rowptr, colidx, val, x, alpha, beta, y);
    if (!csr_args_ok(rows, cols, nnz, rowptr, colidx, val)) return SBLAS_E_INVALID;
    if (!y || (cols > 0 && !x)) return SBLAS_E_INVALID;
    if (const int vrc = validate_if_asked(dev, stream, rows, cols, nnz, rowptr, colidx)) return vrc;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    const hipError_t e = p->pv.as_unplanned
                             ? sblas::launch_spmv((hipStream_t)stream, (int)rows, (int)cols, nnz, rowptr, colidx, val, x, alpha, beta, y)
                             : sblas::launch_spmv_planned((hipStream_t)stream, (int)cols, p->pv, rowptr, colidx, val, x, alpha, beta, y);
    return e == hipSuccess
               ? SBLAS_OK
               : SBLAS_E_HIP;
}

int sblas_hip_axpby_f64(int dev, void *stream, int64_t n, double alpha, const double *x, double beta,
                        double *y)
{
    if (n < 0) return SBLAS_E_INVALID;
    if (n == 0) return SBLAS_OK;
    if (!x || !y) return SBLAS_E_INVALID;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    return sblas::launch_axpby((hipStream_t)stream, n, alpha, x, beta, y) == hipSuccess ? SBLAS_OK
                                                                                       : SBLAS_E_HIP;
}

// ---- the other value / index types (typed_kernels.hip); <int32, fp64> forwards to the tuned entry points above ----
static bool types_ok(int vtype, int itype)
{
    return (vtype == SBLAS_F64 || vtype == SBLAS_F32) && (itype == SBLAS_I32 || itype == SBLAS_I64);
}

size_t sblas_hip_spmm_csr_workspace(int vtype, int itype, int64_t rows, int64_t cols, int64_t nnz, int64_t n)
{
    if (!types_ok(vtype, itype)) return 0;
    if (vtype == SBLAS_F64 && itype == SBLAS_I32) return sblas_hip_spmm_csr_f64_i32_workspace(rows, cols, nnz, n);
    return sblas::typed_spmm_workspace(vtype, cols, n);
}

int sblas_hip_spmm_csr(int dev, void *stream, int vtype, int itype, int64_t rows, int64_t cols, int64_t nnz,
                       const void *rowptr, const void *colidx, const void *val, const void *B, int64_t ldb, int64_t n,
                       double alpha, double beta, void *C, int64_t ldc, void *workspace, size_t workspace_bytes)
{
    return sblas_hip_spmm_csr_ordered(dev, stream, vtype, itype, rows, cols, nnz, rowptr, colidx, val, B, ldb,
                                      SBLAS_COL_MAJOR, n, alpha, beta, C, ldc, SBLAS_COL_MAJOR, workspace, workspace_bytes);
}

int sblas_hip_spmm_csr_ordered(int dev, void *stream, int vtype, int itype, int64_t rows, int64_t cols, int64_t nnz,
                               const void *rowptr, const void *colidx, const void *val, const void *B, int64_t ldb,
                               int order_b, int64_t n, double alpha, double beta, void *C, int64_t ldc, int order_c,
                               void *workspace, size_t workspace_bytes)
{
    if (!types_ok(vtype, itype) || !order_ok(order_b) || !order_ok(order_c)) return SBLAS_E_INVALID;
    if (vtype == SBLAS_F64 && itype == SBLAS_I32)
        return spmm_impl(dev, stream, rows, cols, nnz, static_cast<const int32_t *>(rowptr),
                         static_cast<const int32_t *>(colidx), static_cast<const double *>(val),
                         static_cast<const double *>(B), ldb, order_b, n, alpha, beta, static_cast<double *>(C), ldc,
                         order_c, workspace, workspace_bytes, nullptr);
    if (rows < 0 || cols < 0 || nnz < 0 || n < 0 || !rowptr || (nnz > 0 && (!colidx || !val))) return SBLAS_E_INVALID;
    if (itype == SBLAS_I32 && (rows > INT_MAX - 64 || cols > INT_MAX || nnz > INT_MAX)) return SBLAS_E_INVALID;
    if (rows == 0 || n == 0) return SBLAS_OK;
    if (!C || !ld_ok(order_c, ldc, rows, n)) return SBLAS_E_INVALID;
    if (cols > 0 && (!B || !ld_ok(order_b, ldb, cols, n))) return SBLAS_E_INVALID;
    const size_t need = (cols == 0 || nnz == 0) ? 0 : sblas::typed_spmm_workspace(vtype, cols, n);
    if (need > 0 && (!workspace || workspace_bytes < need)) return SBLAS_E_WORKSPACE;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    return sblas::launch_typed_spmm((hipStream_t)stream, vtype, itype, rows, cols, nnz, rowptr, colidx, val, B, ldb, n, alpha,
                                    beta, C, ldc, workspace, order_b == SBLAS_ROW_MAJOR, order_c == SBLAS_ROW_MAJOR) == hipSuccess
               ? SBLAS_OK
               : SBLAS_E_HIP;
}

int sblas_hip_spmv_csr(int dev, void *stream, int vtype, int itype, int64_t rows, int64_t cols, int64_t nnz,
                       const void *rowptr, const void *colidx, const void *val, const void *x, double alpha,
                       double beta, void *y)
{
    if (!types_ok(vtype, itype)) return SBLAS_E_INVALID;
    if (vtype == SBLAS_F64 && itype == SBLAS_I32)
        return sblas_hip_spmv_csr_f64_i32(dev, stream, rows, cols, nnz, static_cast<const int32_t *>(rowptr),
                                          static_cast<const int32_t *>(colidx), static_cast<const double *>(val),
                                          static_cast<const double *>(x), alpha, beta, static_cast<double *>(y));
    if (rows < 0 || cols < 0 || nnz < 0 || !rowptr || (nnz > 0 && (!colidx || !val))) return SBLAS_E_INVALID;
    if (itype == SBLAS_I32 && (rows > INT_MAX - 64 || cols > INT_MAX || nnz > INT_MAX)) return SBLAS_E_INVALID;
    if (rows == 0) return SBLAS_OK;
    if (!y || (cols > 0 && !x)) return SBLAS_E_INVALID;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    return sblas::launch_typed_spmv((hipStream_t)stream, vtype, itype, rows, rowptr, colidx, val, x, alpha, beta, y) ==
                   hipSuccess
               ? SBLAS_OK
               : SBLAS_E_HIP;
}

int sblas_hip_axpby(int dev, void *stream, int vtype, int64_t n, double alpha, const void *x, double beta, void *y)
{
    if (vtype == SBLAS_F64)
        return sblas_hip_axpby_f64(dev, stream, n, alpha, static_cast<const double *>(x), beta, static_cast<double *>(y));
    if (vtype != SBLAS_F32 || n < 0) return SBLAS_E_INVALID;
    if (n == 0) return SBLAS_OK;
    if (!x || !y) return SBLAS_E_INVALID;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    return sblas::launch_typed_axpby((hipStream_t)stream, vtype, n, alpha, x, beta, y) == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

} // extern "C"
