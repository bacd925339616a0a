// gmres_fold.h -- stage 2 of GMRES's dots, which is also its scalar step: the one text gmres.hip's fold (one workgroup)
// and gmres_multi.hip's fold (one workgroup a column) both run.  A fold is three parts: who acts (block-uniform loads of
// the scalar block, before any barrier), the sums of the cells' partials in the single dot's order, and what lane 0 takes
// from them (h, h + c, or the scalar step of gmres.h: the Givens rotations, |g_{j+1}|, the test, the count, the status).
// The including file switches contraction off ahead of gmres.h, as gmres.hip does.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "gmres.h"
#include "krylov_fold.h"

#pragma clang fp contract(off)

namespace sblas {

// fold ops: what lane 0 does with the folded sums
enum { GF_OUT = 0, GF_START_B, GF_BEGIN_START, GF_BEGIN_RESTART, GF_H1, GF_H2, GF_STEP };

// Who acts.  A fold that opens a sequence says so in GS_ACTIVE; false: the workgroup returns.
__device__ __forceinline__ bool gmres_fold_acts(int op, long long *ib)
{
    if (op == GF_H1 || op == GF_BEGIN_START || op == GF_BEGIN_RESTART) {
        bool act = ib[GS_STATUS] == GMRES_RUNNING;
        if (op == GF_H1) act = act && ib[GS_COLS] < ib[GS_M];
        if (op == GF_BEGIN_RESTART) act = act && ib[GS_COLS] == ib[GS_M] && ib[GS_PENDING] == 0;
        if (!act) {
            if (threadIdx.x == 0) ib[GS_ACTIVE] = 0;
            return false;
        }
    } else if (op == GF_H2 || op == GF_STEP) {
        if (!ib[GS_ACTIVE]) return false;
    }
    return true;
}

// The dots one after another, each as the single dot's second stage: lane t adds partial[t], partial[t + 256], ... in
// order from +0, then the butterfly; dot q's cells' sums start at part + q * stride.  The waves' sums wait in ws for the
// caller's barrier.
__device__ __forceinline__ void gmres_fold_sums(int nd, int64_t cells, const double *part, int64_t stride, double (*ws)[4])
{
    for (int q = 0; q < nd; ++q) {
        double acc = 0.0;
        for (int64_t c = threadIdx.x; c < cells; c += KRYLOV_LANES) acc = acc + part[(int64_t)q * stride + c];
        const double v = wave_fold(acc);
        if ((threadIdx.x & 63) == 0) ws[q][threadIdx.x >> 6] = v;
    }
}

// Lane 0's part.  ws: the waves' sums behind the barrier; out (GF_OUT): dot q to out[q * out_stride].
__device__ __forceinline__ void gmres_fold_lane0(int op, int nd, const double (*ws)[4], double *blk, double *mat, double *out, int64_t out_stride,
                                                 double rtol, double atol, long long max_iter, int m)
{
    long long *ib = reinterpret_cast<long long *>(blk);
    auto d = [&](int q) { return (ws[q][0] + ws[q][1]) + (ws[q][2] + ws[q][3]); };
    double *h = mat + GM_H, *h2 = mat + GM_H2, *g = mat + GM_G;
    switch (op) {
    case GF_OUT:
        for (int q = 0; q < nd; ++q) out[(int64_t)q * out_stride] = d(q);
        break;
    case GF_START_B: {
        const double bnorm = sqrt(d(0)), t = rtol * bnorm;
        blk[GS_RNORM] = 0.0, blk[GS_ETA] = 0.0, blk[GS_BNORM] = bnorm, blk[GS_TOL] = t >= atol ? t : atol;
        ib[GS_ITER] = 0, ib[GS_RESTARTS] = 0, ib[GS_COLS] = 0, ib[GS_WHICH] = 0, ib[GS_PENDING] = 0, ib[GS_MAX_ITER] = max_iter;
        ib[GS_M] = m, ib[GS_CLOSE] = 0, ib[GS_ACTIVE] = 0, ib[15] = 0;
        const bool zero = d(0) == 0.0; // b == 0: x = 0, converged at iteration 0, and nothing is divided
        ib[GS_ZERO_X] = zero, ib[GS_STATUS] = zero ? GMRES_CONVERGED : GMRES_RUNNING;
        break;
    }
    case GF_BEGIN_START:
    case GF_BEGIN_RESTART: {
        const double beta = sqrt(d(0));
        int64_t which = 0;
        const int st = gmres_begin(beta, blk[GS_TOL], (int64_t)ib[GS_ITER], (int64_t)ib[GS_MAX_ITER], &which);
        blk[GS_RNORM] = beta, ib[GS_COLS] = 0, ib[GS_STATUS] = st, ib[GS_WHICH] = which, ib[GS_ACTIVE] = st == GMRES_RUNNING;
        if (op == GF_BEGIN_RESTART) ib[GS_RESTARTS] = ib[GS_RESTARTS] + 1;
        if (st == GMRES_RUNNING) blk[GS_ETA] = beta, g[0] = beta; // g = beta e_1: the step writes g_{j+1} before it is read
        break;
    }
    case GF_H1:
        for (int q = 0; q < nd; ++q) h[q] = d(q);
        ib[GS_ACTIVE] = 1;
        break;
    case GF_H2:
        for (int q = 0; q < nd; ++q) {
            const double cq = d(q);
            h2[q] = cq, h[q] = h[q] + cq;
        }
        break;
    case GF_STEP: {
        const int j = (int)ib[GS_COLS];
        const double eta = sqrt(d(0));
        int64_t iter = (int64_t)ib[GS_ITER], which = 0;
        double rnorm = blk[GS_RNORM];
        const int st = gmres_step(j, h, eta, mat + GM_C, mat + GM_S, g, mat + GM_R + (int64_t)j * GMRES_MAX_RESTART, blk[GS_TOL],
                                  (int64_t)ib[GS_MAX_ITER], &iter, &rnorm, &which);
        blk[GS_ETA] = eta;
        ib[GS_STATUS] = st, ib[GS_ACTIVE] = st == GMRES_RUNNING;
        if (st == GMRES_BREAKDOWN) ib[GS_WHICH] = which; // column j is dropped: the columns before it stay pending
        else ib[GS_ITER] = iter, blk[GS_RNORM] = rnorm, ib[GS_COLS] = j + 1, ib[GS_PENDING] = 1;
        break;
    }
    default: break;
    }
}

// The first kernel of a close, one lane: does it act, and if so y from R y = g over the finished columns.
__device__ __forceinline__ void gmres_close_lane(double *blk, double *mat)
{
    long long *ib = reinterpret_cast<long long *>(blk);
    const int k = (int)ib[GS_COLS];
    const bool act = ib[GS_PENDING] != 0 && (ib[GS_COLS] == ib[GS_M] || ib[GS_STATUS] != GMRES_RUNNING);
    ib[GS_CLOSE] = act;
    if (!act) return;
    gmres_back_substitute(k, mat + GM_R, GMRES_MAX_RESTART, mat + GM_G, mat + GM_Y);
    ib[GS_PENDING] = 0; // applied: a second close changes nothing
}

} // namespace sblas
