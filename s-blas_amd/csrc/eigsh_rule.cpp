// eigsh_rule.cpp -- the host rule of the eigenvalue plan (eigsh.hip): the limits, the launch counts, and
// the cyclic Jacobi loop, the whole Ritz step and the basis rotation restated in plain C++ through the very functions the
// device compiles (eigsh.h).  Pure functions of host arrays; no GPU call in this file, so it is testable on a CPU box (and
// under a host sanitizer).
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/sblas_hip.h"

#pragma clang fp contract(off) // ahead of eigsh.h: every product and every sum below is rounded on its own

#include "eigsh.h"

static_assert(SBLAS_KRYLOV_RUNNING == sblas::EIGSH_RUNNING && SBLAS_KRYLOV_CONVERGED == sblas::EIGSH_CONVERGED &&
                  SBLAS_KRYLOV_BREAKDOWN == sblas::EIGSH_BREAKDOWN && SBLAS_KRYLOV_LIMIT == sblas::EIGSH_LIMIT,
              "eigsh.h restates them");
static_assert(SBLAS_EIGSH_MAX_NCV == sblas::EIGSH_MAX_NCV && SBLAS_EIGSH_BLOCK_SLOTS == sblas::EIGSH_BLOCK_SLOTS &&
                  SBLAS_EIGSH_MATRIX_DOUBLES == sblas::EIGSH_MATRIX_DOUBLES,
              "the header's sizes are eigsh.h's");
static_assert(SBLAS_EIGSH_LA == sblas::EIGSH_LA && SBLAS_EIGSH_SA == sblas::EIGSH_SA && SBLAS_EIGSH_LM == sblas::EIGSH_LM, "eigsh.h restates them");

namespace {

using namespace sblas;

constexpr int LD = EIGSH_LD;

// Cyclic Jacobi over the leading mm x mm of T (64 x 64 by columns, zero outside mm x mm): on return T's diagonal holds
// the eigenvalues and Y (64 x 64 by columns) the eigenvectors by columns.  A round's rotations are all taken from T as
// the round began, then every 2 x 2 block and every row of Y is updated once -- what the device does side by side.
int jacobi(int mm, double *T, double *Y)
{
    const int M = mm + (mm & 1), np = M / 2;
    std::vector<double> next((size_t)LD * LD);
    memset(Y, 0, sizeof(double) * LD * LD);
    for (int i = 0; i < mm; ++i) Y[i * LD + i] = 1.0;
    int sweeps = 0;
    for (; sweeps < EIGSH_MAX_SWEEPS; ++sweeps) {
        bool rotated = false;
        for (int r = 0; r < M - 1; ++r) {
            int p[LD / 2], q[LD / 2];
            double c[LD / 2], s[LD / 2], dpp[LD / 2], dqq[LD / 2];
            for (int i = 0; i < np; ++i) {
                eigsh_pair(M, r, i, &p[i], &q[i]);
                if (eigsh_rotation(T[p[i] * LD + p[i]], T[q[i] * LD + q[i]], T[q[i] * LD + p[i]], &c[i], &s[i], &dpp[i], &dqq[i])) rotated = true;
            }
            memcpy(next.data(), T, sizeof(double) * LD * LD);
            for (int bi = 0; bi < np; ++bi)
                for (int bj = 0; bj < np; ++bj) {
                    const int p1 = p[bi], q1 = q[bi], p2 = p[bj], q2 = q[bj];
                    double bpp = T[p2 * LD + p1], bpq = T[q2 * LD + p1], bqp = T[p2 * LD + q1], bqq = T[q2 * LD + q1];
                    if (bi == bj) bpp = dpp[bi], bqq = dqq[bi], bpq = 0.0, bqp = 0.0;
                    else eigsh_block(bi < bj, c[bi], s[bi], c[bj], s[bj], &bpp, &bpq, &bqp, &bqq);
                    next[p2 * LD + p1] = bpp, next[q2 * LD + p1] = bpq, next[p2 * LD + q1] = bqp, next[q2 * LD + q1] = bqq;
                }
            memcpy(T, next.data(), sizeof(double) * LD * LD);
            for (int i = 0; i < np; ++i)
                for (int row = 0; row < mm; ++row) eigsh_rotate_pair(c[i], s[i], &Y[p[i] * LD + row], &Y[q[i] * LD + row]);
        }
        if (!rotated) break;
    }
    return sweeps;
}

bool finite_block(int mm, const double *T)
{
    for (int c = 0; c < mm; ++c)
        for (int r = 0; r < mm; ++r)
            if (!isfinite(T[c * LD + r])) return false;
    return true;
}

} // namespace

extern "C" {

int sblas_eigsh_limits(int64_t out[16])
{
    if (!out) return SBLAS_E_INVALID;
    out[0] = EIGSH_MAX_NCV, out[1] = EIGSH_DEFAULT_NCV, out[2] = EIGSH_LD, out[3] = EIGSH_MAX_SWEEPS, out[4] = EIGSH_BLOCK_SLOTS;
    out[5] = EIGSH_MATRIX_DOUBLES, out[6] = EM_T, out[7] = EM_Y, out[8] = EM_THETA, out[9] = EM_RHO, out[10] = EM_Q, out[11] = EM_H, out[12] = EM_C;
    out[13] = EIGSH_ROTATE_THREADS, out[14] = EIGSH_RITZ_THREADS, out[15] = 0;
    return SBLAS_OK;
}

int sblas_eigsh_sizes(int64_t n, int k, int ncv, int keep, int64_t out[2])
{
    if (!out || k < 1) return SBLAS_E_INVALID;
    if (ncv <= 0) ncv = eigsh_default_ncv(n, k);
    if (keep <= 0) keep = eigsh_default_keep(k, ncv);
    out[0] = ncv, out[1] = keep;
    return eigsh_sizes_ok(n, k, ncv, keep) ? SBLAS_OK : SBLAS_E_INVALID;
}

int64_t sblas_eigsh_launches(int ncv, int keep, int64_t out[4])
{
    if (!out || ncv < 2 || ncv > EIGSH_MAX_NCV || keep < 1 || keep > ncv - 1) return -1;
    // step: SpMV; multi-dot, fold; projection; multi-dot, fold; projection with (w, w); fold and T's column; normalisation
    out[0] = 9;
    out[1] = 3 + 9 * (int64_t)keep;         // start: v0 with (v0, v0); fold; normalisation; the first `keep` steps
    out[2] = 9 * (int64_t)(ncv - keep) + 2; // cycle: steps keep .. ncv - 1; the Ritz kernel; the rotation
    out[3] = 2;
    return out[2];
}

int sblas_eigsh_jacobi_ref(int mm, const double *T, int ldt, double *theta, double *Y, int ldy, int *sweeps)
{
    if (mm < 1 || mm > EIGSH_MAX_NCV || !T || ldt < mm || !theta || !Y || ldy < mm) return SBLAS_E_INVALID;
    std::vector<double> t((size_t)LD * LD, 0.0), y((size_t)LD * LD);
    for (int c = 0; c < mm; ++c)
        for (int r = 0; r < mm; ++r) t[c * LD + r] = T[(int64_t)c * ldt + r];
    const int done = jacobi(mm, t.data(), y.data());
    if (sweeps) *sweeps = done;
    for (int c = 0; c < mm; ++c) {
        theta[c] = t[c * LD + c];
        for (int r = 0; r < mm; ++r) Y[(int64_t)c * ldy + r] = y[c * LD + r];
    }
    return SBLAS_OK;
}

int sblas_eigsh_ritz_ref(int k, int keep, int which, double *blk, double *mat)
{
    if (!blk || !mat || !eigsh_which_ok(which) || k < 1 || keep < k || keep > EIGSH_MAX_NCV - 1) return SBLAS_E_INVALID;
    int64_t *ib = reinterpret_cast<int64_t *>(blk);
    const int64_t cols = ib[ES_COLS];
    if (cols < 1 || cols > EIGSH_MAX_NCV) return SBLAS_E_INVALID;
    if (ib[ES_STATUS] != EIGSH_RUNNING) { // the freeze: only the flag of the rotation falls
        ib[ES_ACT] = 0;
        return SBLAS_OK;
    }
    const int mm = (int)cols, kk = keep < mm ? keep : mm;
    double *T = mat + EM_T, *Y = mat + EM_Y, *theta = mat + EM_THETA, *rho = mat + EM_RHO, *Q = mat + EM_Q;
    if (!finite_block(mm, T)) {
        ib[ES_STATUS] = EIGSH_BREAKDOWN, ib[ES_WHICH] = EIGSH_DENOM_T, ib[ES_ACT] = 0;
        return SBLAS_OK;
    }
    std::vector<double> t((size_t)LD * LD, 0.0);
    for (int c = 0; c < mm; ++c)
        for (int r = 0; r < mm; ++r) t[c * LD + r] = T[c * LD + r];
    jacobi(mm, t.data(), Y);
    int order[EIGSH_MAX_NCV];
    for (int i = 0; i < EIGSH_MAX_NCV; ++i) order[i] = i; // values that do not order (a NaN from an overflow) leave no entry unwritten
    for (int i = 0; i < mm; ++i) {
        int rank = 0;
        for (int j = 0; j < mm; ++j)
            if (j != i && eigsh_before(which, t[j * LD + j], j, t[i * LD + i], i)) ++rank;
        order[rank] = i;
    }
    const double beta = blk[ES_BETA];
    int met = 0;
    for (int r = 0; r < mm; ++r) {
        const int i = order[r];
        theta[r] = t[i * LD + i];
        rho[r] = fabs(beta * Y[i * LD + (mm - 1)]);
        if (r < k && eigsh_met(rho[r], theta[r], blk[ES_RTOL], blk[ES_ATOL])) ++met;
    }
    for (int r = 0; r < kk; ++r)
        for (int l = 0; l < mm; ++l) Q[r * LD + l] = Y[order[r] * LD + l];
    for (int e = 0; e < LD * LD; ++e) T[e] = 0.0;
    for (int r = 0; r < kk; ++r) T[r * LD + r] = theta[r];
    int64_t which_out = 0;
    ib[ES_RESTARTS] = ib[ES_RESTARTS] + 1;
    ib[ES_STATUS] = eigsh_decide(mm, k, met, ib[ES_INVARIANT] != 0, ib[ES_RESTARTS], ib[ES_MAX_RESTARTS], &which_out);
    ib[ES_WHICH] = which_out, ib[ES_CONVERGED] = met, ib[ES_COLS] = kk, ib[ES_MM] = mm, ib[ES_KK] = kk, ib[ES_ACT] = 1;
    return SBLAS_OK;
}

int sblas_eigsh_step_ref(int j, const double *h, double beta, double *blk, double *mat)
{
    if (j < 0 || j >= EIGSH_MAX_NCV || !h || !blk || !mat) return -1;
    return eigsh_step(j, h, beta, mat + EM_T, blk) ? 1 : 0;
}

int sblas_eigsh_rotate_ref(int64_t n, int mm, int keep, double *V, int64_t ldv, const double *Q, int ldq)
{
    if (n < 0 || mm < 1 || mm > EIGSH_MAX_NCV || keep < 1 || keep > mm || ldv < n || ldq < mm || !Q || (n > 0 && !V)) return SBLAS_E_INVALID;
    double v[EIGSH_MAX_NCV + 1];
    for (int64_t row = 0; row < n; ++row) {
        for (int l = 0; l <= mm; ++l) v[l] = V[l * ldv + row];
        for (int i = 0; i < keep; ++i) {
            double acc = Q[(int64_t)i * ldq] * v[0];
            for (int l = 1; l < mm; ++l) acc = acc + Q[(int64_t)i * ldq + l] * v[l];
            V[i * ldv + row] = acc;
        }
        V[keep * ldv + row] = v[mm];
    }
    return SBLAS_OK;
}

} // extern "C"
