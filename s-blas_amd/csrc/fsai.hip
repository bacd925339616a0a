// fsai.hip -- the factorised sparse approximate inverse of Kolotilina and Yeremin on a device plan: for a
// symmetric positive definite CSR matrix A with fp64 values, int32 indices, strictly ascending rows and a stored diagonal,
// a sparse lower-triangular G with G A G^T ~ I, applied as z = G^T (G r).
//
// create is host work, as the Chebyshev plan's: the structure comes to the host once, sblas_fsai_pattern checks it and
// gives G's pattern (A's lower part or the caller's, thinned to max_row), the rows are packed into four-lane units as one
// wide level of a solve, and the plan makes an SpMV plan on G and a transpose plan (with its SpMV plan) on G.  setup is ONE
// launch of one kernel and the transpose plan's value update; apply is the two planned SpMVs.  Nothing waits across
// workgroups, nothing inside one either: a row of G lives in the lanes of one wave, which order their LDS traffic
// themselves.  The only atomic is the integer minimum of the failed-row word, the same in every order.
//
// The kernel.  Row i of G with m entries J is worked by G(m) lanes, the solves' group rule, and owns those lanes' share of
// the workgroup's LDS: the packed lower triangle of M (row after row), J, and a vector that first holds the extents of
// A's rows J[p] and later g.
//   gather   M[p][q] = A[J[p]][J[q]]: the triangle is cleared to +0; then for every p the group's lanes run along A's row
//            J[p] up to its diagonal, coalesced, and a binary search in J[0 .. p] places what they meet.  Exact.
//   factor   right-looking Cholesky in place.  Step k: every lane reads the pivot; the lanes divide column k (lane l the
//            rows k + 1 + l, + G); then lane l holds M[q][k] of its columns q = k + 1 + l (+ G) in registers and the
//            group walks the rows p = k + 1 .. m - 1 together: M[p][k] is one broadcast read and row p's entries are
//            consecutive words.  A pivot that is not finite and > 0 fails the whole row, uniformly over its lanes.
//   solve    C^T g = e_m column by column: lane l carries t[l] (and t[l + G]) in registers, g[q] is a broadcast read.
//   store    g to val_G, coalesced; a failed row as its diagonal alone, and its number into the flag.
// Every entry of M takes its updates in ascending k and every t[p] in descending q, one rounding an operation, so the
// bits are the scalar loop's (fsai_rule.cpp) under every schedule: contraction is off.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <memory>
#include <vector>
#include "../../include/sblas_hip.h"
#define FSAI_HD __host__ __device__
#include "fsai.h"
#include "level_kernels.h"

#pragma clang fp contract(off) // file scope: a - b * c below is two roundings

using namespace sblas;

namespace {

// orders the LDS traffic of one wave's lanes: what a lane wrote before is what another lane of the wave reads after
__device__ __forceinline__ void step_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(FSAI_THREADS) void fsai_setup_kernel(int64_t count, const FsaiUnit *__restrict__ units, const int32_t *__restrict__ rowptr,
                                                                  const int32_t *__restrict__ colidx, const double *__restrict__ val,
                                                                  const int32_t *__restrict__ colidx_g, double *__restrict__ val_g,
                                                                  unsigned long long *flag)
{
    __shared__ double tri[FSAI_THREADS * FSAI_TRI_PER_LANE];
    __shared__ long long vec[FSAI_THREADS * FSAI_VEC_PER_LANE]; // the rows' extents (two int32 a word), then g's bits
    __shared__ int32_t cols[FSAI_THREADS * FSAI_VEC_PER_LANE];
    const FsaiUnit u = wide_unit<FSAI_THREADS>(0, count, units, NO_FSAI_UNIT);
    if (u.row < 0) return; // whole groups leave together: nothing below crosses a group
    const int m = u.end - u.beg;
    // the lane's place in its row is its place in the workgroup modulo G: the plan aligns a row to G lanes of the launch
    const int G = 1 << sptrsv_group_shift(m), ln = (int)threadIdx.x & (G - 1), first = (int)threadIdx.x - ln;
    double *M = tri + first * FSAI_TRI_PER_LANE;
    long long *w = vec + first * FSAI_VEC_PER_LANE;
    int32_t *J = cols + first * FSAI_VEC_PER_LANE;

    // ---- gather --------------------------------------------------------------------------------------------------------
    for (int e = ln; e < m; e += G) {
        const int32_t r = colidx_g[(int64_t)u.beg + e];
        J[e] = r;
        w[e] = (long long)(((unsigned long long)(uint32_t)rowptr[r + 1] << 32) | (uint32_t)rowptr[r]);
    }
    for (int e = ln; e < fsai_triangle(m); e += G) M[e] = 0.0;
    step_fence();
    for (int p = 0; p < m; ++p) {
        const int32_t r = J[p];
        const unsigned long long ext = (unsigned long long)w[p];
        const int64_t end = (int64_t)(ext >> 32);
        for (int64_t e = (int64_t)(uint32_t)ext + ln; e < end; e += G) {
            const int32_t c = colidx[e];
            if (c > r) break; // the row ascends: only entries with column <= row are read
            int lo = 0, hi = p + 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (J[mid] < c) lo = mid + 1;
                else hi = mid;
            }
            if (lo <= p && J[lo] == c) M[fsai_at(p, lo)] = val[e];
        }
    }
    step_fence();

    // ---- factor --------------------------------------------------------------------------------------------------------
    const double aii = M[fsai_at(m - 1, m - 1)];
    bool ok = true;
    for (int k = 0; k < m; ++k) {
        const double d = M[fsai_at(k, k)];
        if (!fsai_positive(d)) { // the same in every lane of the row
            ok = false;
            break;
        }
        const double c = sqrt(d);
        step_fence(); // the pivot was read by every lane
        if (ln == 0) M[fsai_at(k, k)] = c;
        for (int p = k + 1 + ln; p < m; p += G) M[fsai_at(p, k)] = M[fsai_at(p, k)] / c;
        step_fence();
        // at most two columns a lane: m - k - 1 <= 2 G in every tier (fsai.h)
        const int q0 = k + 1 + ln, q1 = q0 + G;
        const double l0 = q0 < m ? M[fsai_at(q0, k)] : 0.0, l1 = q1 < m ? M[fsai_at(q1, k)] : 0.0;
        for (int p = k + 1; p < m; ++p) {
            const double lp = M[fsai_at(p, k)];
            if (q0 <= p) {
                const double prod = lp * l0;
                M[fsai_at(p, q0)] = M[fsai_at(p, q0)] - prod;
            }
            if (q1 <= p) {
                const double prod = lp * l1;
                M[fsai_at(p, q1)] = M[fsai_at(p, q1)] - prod;
            }
        }
        step_fence();
    }

    if (!ok) { // the diagonal alone
        const double fallback = fsai_positive(aii) ? 1.0 / sqrt(aii) : 1.0;
        for (int e = ln; e < m; e += G) val_g[(int64_t)u.beg + e] = e == m - 1 ? fallback : 0.0;
        if (ln == 0) atomicMin(flag, (unsigned long long)u.row);
        return;
    }

    // ---- solve ---------------------------------------------------------------------------------------------------------
    double t0 = 0.0, t1 = 0.0; // t[ln], t[ln + G]
    step_fence();              // the extents were read out
    if (ln == 0) w[m - 1] = __double_as_longlong(1.0 / M[fsai_at(m - 1, m - 1)]);
    step_fence();
    for (int q = m - 1; q >= 1; --q) {
        const double gq = __longlong_as_double(w[q]);
        if (ln < q) {
            const double prod = M[fsai_at(q, ln)] * gq;
            t0 = t0 + prod;
        }
        if (ln + G < q) {
            const double prod = M[fsai_at(q, ln + G)] * gq;
            t1 = t1 + prod;
        }
        if (ln == ((q - 1) & (G - 1))) {
            const double tq = q - 1 >= G ? t1 : t0;
            w[q - 1] = __double_as_longlong((-tq) / M[fsai_at(q - 1, q - 1)]);
        }
        step_fence();
    }
    for (int e = ln; e < m; e += G) val_g[(int64_t)u.beg + e] = __longlong_as_double(w[e]);
}

struct FsaiPlan {
    int dev = -1;
    int64_t n = 0, nnz = 0, nnz_g = 0, longest = 0, units = 0, tiers[3] = {0, 0, 0};
    const int32_t *rowptr = nullptr, *colidx = nullptr; // the caller's A
    DeviceBuffer ibuf, dbuf;                            // units | G's rowptr | G's colidx;  val_G | t | flag
    const FsaiUnit *d_units = nullptr;
    const int32_t *rowptr_g = nullptr, *colidx_g = nullptr;
    double *val_g = nullptr, *t = nullptr;
    unsigned long long *flag = nullptr;
    void *spmv = nullptr, *transpose = nullptr; // the SpMV plan on G; the transpose plan on G with its SpMV plan
    size_t bytes = 0;
    bool ready = false; // setup's
    ~FsaiPlan()
    {
        if (transpose) sblas_hip_transpose_plan_destroy(transpose);
        if (spmv) sblas_hip_spmv_plan_destroy(spmv);
    }
};

bool overlap(const double *a, const double *b, int64_t n) { return a < b + n && b < a + n; }

} // namespace

extern "C" {

int sblas_hip_fsai_plan_create(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx, int64_t nnz_g,
                               const int32_t *rowptr_g, const int32_t *colidx_g, int max_row, void **plan_out, int64_t *bad_row)
{
    if (bad_row) *bad_row = -1;
    if (!plan_out) return SBLAS_E_INVALID;
    *plan_out = nullptr;
    if (!fsai_max_row_ok(max_row)) return SBLAS_E_INVALID;
    if (n < 0 || nnz < 0 || n > INT_MAX - 64 || nnz > INT_MAX || (n == 0 && nnz != 0)) return SBLAS_E_INVALID;
    if ((n > 0 && !rowptr) || (nnz > 0 && !colidx)) return SBLAS_E_INVALID;
    const bool own = rowptr_g != nullptr;
    if (own ? (nnz_g < 0 || nnz_g > INT_MAX || (nnz_g > 0 && !colidx_g) || (n == 0 && nnz_g != 0)) : (nnz_g != 0 || colidx_g != nullptr))
        return SBLAS_E_INVALID;
    std::unique_ptr<FsaiPlan> p(new FsaiPlan);
    p->dev = resolve_device(dev), p->n = n, p->nnz = nnz, p->rowptr = rowptr, p->colidx = colidx;
    if (n == 0) {
        *plan_out = p.release();
        return SBLAS_OK;
    }
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int32_t> h_rowptr, h_colidx, h_rowptr_p, h_colidx_p;
    int rc = fetch_structure(s, n, nnz, rowptr, colidx, h_rowptr, h_colidx, bad_row);
    if (rc == SBLAS_OK && own) rc = fetch_structure(s, n, nnz_g, rowptr_g, colidx_g, h_rowptr_p, h_colidx_p, bad_row);
    if (rc != SBLAS_OK) return rc;
    std::vector<int32_t> g_rowptr((size_t)n + 1), g_colidx((size_t)(own ? nnz_g : nnz));
    rc = sblas_fsai_pattern(n, h_rowptr.data(), h_colidx.data(), nnz_g, own ? h_rowptr_p.data() : nullptr, own ? h_colidx_p.data() : nullptr, max_row,
                            g_rowptr.data(), g_colidx.data(), bad_row);
    if (rc != SBLAS_OK) return rc;
    p->nnz_g = g_rowptr[(size_t)n];
    g_colidx.resize((size_t)p->nnz_g);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t m = (int64_t)g_rowptr[(size_t)i + 1] - g_rowptr[(size_t)i];
        const int gs = sptrsv_group_shift(m);
        if (m > p->longest) p->longest = m;
        ++p->tiers[gs == 2 ? 0 : gs == 4 ? 1 : 2];
    }
    // the rows packed as one wide level of a solve, on G's rowptr: a row's lanes go by its length in G
    std::vector<int32_t> zero_level((size_t)n, 0);
    LevelOrder o;
    std::vector<FsaiUnit> units;
    const auto unit_of = [&](int32_t i, int32_t q) { return FsaiUnit{i, g_rowptr[(size_t)i], g_rowptr[(size_t)i + 1], q}; };
    level_pack(n, g_rowptr.data(), zero_level.data(), 1, unit_of, NO_FSAI_UNIT, o, units);
    p->units = (int64_t)units.size();
    Segment seg[3] = {Segment(units), Segment(g_rowptr), Segment(g_colidx)};
    size_t ib = 0;
    if (upload_segments(p->ibuf, p->dev, s, seg, 3, &ib) != hipSuccess) return SBLAS_E_HIP;
    p->d_units = p->ibuf.at<FsaiUnit>(), p->rowptr_g = p->ibuf.at<int32_t>(seg[1].offset), p->colidx_g = p->ibuf.at<int32_t>(seg[2].offset);
    const size_t vb = pad256((size_t)p->nnz_g * 8), tb = pad256((size_t)n * 8), db = vb + tb + 256;
    if (p->dbuf.alloc(p->dev, db) != hipSuccess) return SBLAS_E_HIP;
    p->val_g = p->dbuf.at<double>(), p->t = p->dbuf.at<double>(vb), p->flag = p->dbuf.at<unsigned long long>(vb + tb);
    if (hipMemsetAsync(p->val_g, 0, db, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return SBLAS_E_HIP;
    rc = sblas_hip_spmv_plan_create(dev, stream, n, n, p->nnz_g, p->rowptr_g, p->colidx_g, &p->spmv);
    if (rc == SBLAS_OK) rc = sblas_hip_transpose_plan_create(dev, stream, n, n, p->nnz_g, p->rowptr_g, p->colidx_g, p->val_g, 0, 0, &p->transpose);
    if (rc != SBLAS_OK) return rc;
    int64_t ti[8] = {0};
    sblas_hip_transpose_plan_info(p->transpose, ti);
    p->bytes = ib + db + (size_t)ti[2];
    *plan_out = p.release();
    return SBLAS_OK;
}

int sblas_hip_fsai_plan_info(const void *plan, int64_t out[12])
{
    if (!plan || !out) return SBLAS_E_INVALID;
    const FsaiPlan *p = static_cast<const FsaiPlan *>(plan);
    out[0] = p->n, out[1] = p->nnz, out[2] = p->nnz_g, out[3] = p->longest, out[4] = p->units, out[5] = 2, out[6] = (int64_t)p->bytes;
    out[7] = p->ready, out[8] = p->tiers[0], out[9] = p->tiers[1], out[10] = p->tiers[2], out[11] = 0;
    return SBLAS_OK;
}

int sblas_hip_fsai_plan_speaks_for(const void *plan, int dev, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx)
{
    const FsaiPlan *p = static_cast<const FsaiPlan *>(plan);
    if (!p || p->dev != resolve_device(dev)) return SBLAS_E_INVALID;
    return n == p->n && nnz == p->nnz && rowptr == p->rowptr && colidx == p->colidx ? SBLAS_OK : SBLAS_E_INVALID;
}

int sblas_hip_fsai_plan_destroy(void *plan)
{
    delete static_cast<FsaiPlan *>(plan);
    return SBLAS_OK;
}

int sblas_hip_fsai_plan_csr(const void *plan, const int32_t **rowptr_g, const int32_t **colidx_g, const double **val_g)
{
    const FsaiPlan *p = static_cast<const FsaiPlan *>(plan);
    if (!p) return SBLAS_E_INVALID;
    if (rowptr_g) *rowptr_g = p->rowptr_g;
    if (colidx_g) *colidx_g = p->colidx_g;
    if (val_g) *val_g = p->val_g;
    return SBLAS_OK;
}

int sblas_hip_fsai_plan_setup(void *plan, void *stream, const double *val)
{
    FsaiPlan *p = static_cast<FsaiPlan *>(plan);
    if (!p) return SBLAS_E_INVALID;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    if (p->n > 0 && !val) return SBLAS_E_INVALID;
    p->ready = false;
    if (p->n == 0) {
        p->ready = true;
        return SBLAS_OK;
    }
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(p->flag, 0xff, 8, s) != hipSuccess) return SBLAS_E_HIP;
    fsai_setup_kernel<<<wide_grid(4 * p->units, FSAI_THREADS), FSAI_THREADS, 0, s>>>(p->units, p->d_units, p->rowptr, p->colidx, val, p->colidx_g,
                                                                                     p->val_g, p->flag);
    if (hipGetLastError() != hipSuccess) return SBLAS_E_HIP;
    const int rc = sblas_hip_transpose_plan_update_values(p->transpose, stream, p->val_g);
    if (rc != SBLAS_OK) return rc;
    p->ready = true;
    return SBLAS_OK;
}

int sblas_hip_fsai_plan_apply(const void *plan, void *stream, const double *r, double *z)
{
    const FsaiPlan *p = static_cast<const FsaiPlan *>(plan);
    if (!p || !p->ready) return SBLAS_E_INVALID;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    if (p->n == 0) return SBLAS_OK;
    if (!r || !z || overlap(r, z, p->n)) return SBLAS_E_INVALID;
    const int rc = sblas_hip_spmv_csr_f64_i32_planned(p->spmv, -1, stream, p->n, p->n, p->nnz_g, p->rowptr_g, p->colidx_g, p->val_g, r, 1.0, 0.0, p->t);
    if (rc != SBLAS_OK) return rc;
    return sblas_hip_spmv_csr_t_f64_i32_planned(p->transpose, -1, stream, p->t, 1.0, 0.0, z);
}

int sblas_hip_fsai_plan_check(const void *plan, void *stream, int64_t *bad_row)
{
    const FsaiPlan *p = static_cast<const FsaiPlan *>(plan);
    if (!p || !bad_row || !p->ready) return SBLAS_E_INVALID;
    *bad_row = -1;
    if (p->n == 0) return SBLAS_OK;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    unsigned long long h = ~0ull;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(&h, p->flag, 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return SBLAS_E_HIP;
    if (h != ~0ull) *bad_row = (int64_t)h;
    return SBLAS_OK;
}

} // extern "C"
