// multi_plan.h -- what the multi-right-hand-side solver plans (krylov_multi.hip, gmres_multi.hip) share on the host: the
// fields of a plan, the steps of create (bind the structure and the seat, lay out and allocate the one buffer), the
// planned SpMM, the refusals of start and the read-back of status.  A plan derives from MultiPlanBase
// and keeps what is its own: its sizes and block accessors, its kernels and the order it enqueues them in.  No kernel in
// here.  Internal to each translation unit, as precond.h.
#pragma once
#include <string.h>
#include <initializer_list>
#include "capi_util.h"
#include "krylov_multi.h"
#include "precond.h"

namespace {

struct MultiPlanBase {
    int dev = -1, s = 0;
    int64_t n = 0, nnz = 0, cells = 0;
    const int32_t *rowptr = nullptr, *colidx = nullptr; // the caller's
    void *spmm = nullptr;                               // the plan's own, for width s
    PrecondSeat pre;                                    // start() gives it the caller's values
    int n_blocks = 0;
    size_t block_bytes = 0, partial_bytes = 0, scalar_bytes = 0, ws_bytes = 0, bytes = 0;
    DeviceBuffer buf; // the plan's sections, each padded to 256 bytes, in the order its create lists them
    double *blk = nullptr, *part = nullptr, *ws = nullptr, *vec = nullptr;
    // one solve: start() keeps what iterate() needs
    bool started = false;
    const double *val = nullptr;
    double *x = nullptr;
    int64_t ldx = 0;
    ~MultiPlanBase()
    {
        if (spmm) sblas_hip_spmm_plan_destroy(spmm);
    }
};

// create, behind the wrapper's own refusals: the structure, the device, the seat, and the SpMM plan of a system that is
// not empty.  A kind with a block apply of its own (precond_multi_applied) is seated and its level vectors are reserved
// for nrhs columns; every other kind is seated with the plans it was given, NONE and JACOBI with none.
inline int multi_bind(MultiPlanBase *p, int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx, int nrhs,
                      int precond, const void *lower_plan, const void *upper_plan)
{
    if (n < 0 || nnz < 0 || n > INT_MAX - 64 || nnz > INT_MAX) return SBLAS_E_INVALID;
    if (!rowptr || (nnz > 0 && !colidx) || (n == 0 && nnz != 0)) return SBLAS_E_INVALID;
    const int device = resolve_device(dev);
    p->dev = device, p->s = nrhs, p->n = n, p->nnz = nnz, p->cells = sblas::krylov_cells(n);
    p->rowptr = rowptr, p->colidx = colidx;
    if (sblas::precond_multi_applied(precond)) {
        int64_t info[12];
        if (n == 0 && sblas_hip_amg_plan_info(lower_plan, info) == SBLAS_OK && info[0] == 0) {
            // an empty structure has no content to compare and an empty plan no device memory: it is seated as it is
            p->pre.kind = precond, p->pre.lower = lower_plan, p->pre.rowptr = rowptr, p->pre.colidx = colidx;
        } else if (p->pre.bind(precond, lower_plan, nullptr, device, n, nnz, rowptr, colidx) != SBLAS_OK) {
            return SBLAS_E_INVALID;
        }
        DeviceScope scope(dev);
        if (scope.err != hipSuccess) return SBLAS_E_HIP;
        const int rc = sblas_hip_amg_plan_reserve_multi(const_cast<void *>(lower_plan), stream, nrhs);
        if (rc != SBLAS_OK) return rc;
    } else if (p->pre.bind(precond, lower_plan, upper_plan, device, n, nnz, rowptr, colidx) != SBLAS_OK) {
        return SBLAS_E_INVALID;
    }
    if (n == 0) return SBLAS_OK;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    return sblas_hip_spmm_plan_create(device, stream, n, n, nnz, rowptr, colidx, nrhs, &p->spmm);
}

// a section of the plan's buffer: `count` parts of `raw` bytes, each padded to 256
struct Section {
    double **at;   // where it begins; NULL for a section of no bytes
    size_t *bytes; // the padded size of one part
    size_t raw;
    int count;
};

// create, behind multi_bind: sizes the sections in the order given, allocates them as one buffer and writes it whole,
// the one moment that happens outside a solve, so that no kernel ever reads a value nobody wrote.  Nothing for an empty
// system.  A failed allocation leaves no HIP error behind.
inline int multi_layout(MultiPlanBase *p, void *stream, std::initializer_list<Section> sections)
{
    if (p->n == 0) return SBLAS_OK;
    for (const Section &q : sections) *q.bytes = pad256(q.raw), p->bytes += (size_t)q.count * *q.bytes;
    DeviceScope scope(p->dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    if (p->buf.alloc(p->dev, p->bytes) != hipSuccess) { // the plan and its SpMM plan go with p
        (void)hipGetLastError();
        return SBLAS_E_HIP;
    }
    size_t at = 0;
    for (const Section &q : sections) *q.at = *q.bytes ? p->buf.at<double>(at) : nullptr, at += (size_t)q.count * *q.bytes;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(p->buf.at<char>(), 0, p->bytes, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return SBLAS_E_HIP;
    return SBLAS_OK;
}

// the SpMM's workspace, as a section
inline Section multi_workspace(MultiPlanBase *p) { return {&p->ws, &p->ws_bytes, sblas_hip_spmm_csr_f64_i32_workspace(p->n, p->n, p->nnz, p->s), 1}; }

// out = A in: ONE planned SpMM, both blocks row-major, alpha 1 and beta 0
inline int product(const MultiPlanBase *p, hipStream_t st, const double *in, int64_t ldin, double *out)
{
    return sblas_hip_spmm_csr_ordered_f64_i32_planned(p->spmm, p->dev, st, p->n, p->n, p->nnz, p->rowptr, p->colidx, p->val, in, ldin,
                                                      SBLAS_ROW_MAJOR, p->s, 1.0, 0.0, out, p->s, SBLAS_ROW_MAJOR, p->ws, p->ws_bytes);
}

// start, ahead of the first launch.  MULTI_REFUSED: SBLAS_E_INVALID, and the plan is not started; MULTI_EMPTY: the
// empty system, started, nothing to enqueue; MULTI_GO: the seat has its values, the plan has val, X and ldx, and the
// caller sets started behind its launches.
enum MultiStart { MULTI_REFUSED, MULTI_EMPTY, MULTI_GO };

inline MultiStart multi_start(MultiPlanBase *p, const double *val, const double *lu_or_dinv, const double *B, int64_t ldb, double *X, int64_t ldx,
                              double rtol, double atol, int64_t max_iter)
{
    if (!p) return MULTI_REFUSED;
    if (p->dev != resolve_device(-1)) return MULTI_REFUSED;
    if (!(rtol >= 0.0) || !(atol >= 0.0) || max_iter < 0) return MULTI_REFUSED; // a NaN tolerance is refused too
    if (ldb < p->s || ldx < p->s) return MULTI_REFUSED;
    p->started = p->n == 0;
    if (p->n == 0) return MULTI_EMPTY;
    if (sblas::precond_multi_applied(p->pre.kind)) { // the block cycle needs a plan that is set up, with a smoother that has a block form
        int64_t info[12];
        if (sblas_hip_amg_plan_info(p->pre.lower, info) != SBLAS_OK || !info[10] || info[9] == SBLAS_AMG_CHEBYSHEV) return MULTI_REFUSED;
    }
    if (!B || !X || (p->nnz > 0 && !val) || !p->pre.take(lu_or_dinv)) return MULTI_REFUSED;
    if ((reinterpret_cast<uintptr_t>(B) | reinterpret_cast<uintptr_t>(X)) & 7u) return MULTI_REFUSED;
    if (sblas::blocks_overlap(reinterpret_cast<uintptr_t>(X), ldx, reinterpret_cast<uintptr_t>(B), ldb, p->n, p->s)) return MULTI_REFUSED;
    p->val = val, p->x = X, p->ldx = ldx;
    return MULTI_GO;
}

// status: out[8 * c ..] of column c from the eight slots `table` names of its scalar block of SLOTS eight-byte slots,
// after ONE copy of all blocks and a synchronise.  An integer slot is read as the int64 it holds.
struct StatusSlot {
    int slot;
    bool integer;
};

template <int SLOTS> int multi_status(const MultiPlanBase *p, void *stream, double *out, const StatusSlot (&table)[8])
{
    if (!p || !out || !p->started) return SBLAS_E_INVALID;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    for (int q = 0; q < 8 * p->s; ++q) out[q] = 0.0;
    if (p->n == 0) {
        for (int c = 0; c < p->s; ++c) out[8 * c] = SBLAS_KRYLOV_CONVERGED;
        return SBLAS_OK;
    }
    double h[SBLAS_KRYLOV_MULTI_MAX_RHS * SLOTS];
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = (size_t)p->s * SLOTS * 8;
    if (hipMemcpyAsync(h, p->blk, bytes, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return SBLAS_E_HIP;
    for (int c = 0; c < p->s; ++c) {
        for (int k = 0; k < 8; ++k) {
            const double *v = h + (size_t)c * SLOTS + table[k].slot;
            long long iv;
            memcpy(&iv, v, 8);
            out[8 * c + k] = table[k].integer ? (double)iv : *v;
        }
    }
    return SBLAS_OK;
}

} // namespace
