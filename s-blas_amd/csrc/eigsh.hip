// eigsh.hip -- thick-restart Lanczos (Wu and Simon) with full reorthogonalisation for a few extremal eigenpairs of a
// symmetric CSR matrix, on a device-resident plan, in the style of gmres.hip: start / iterate / status,
// only status synchronises, no atomics, nothing waits across workgroups, no allocation after create, every bit pinned.
// A step at column j is GMRES's step without M^-1:
//   SpMV     w = A v_j (it always runs: a surplus step's product lands in w and nowhere else);
//   dots     stage 1 of (v_i, w), i <= j, in one pass, each with krylov_dot's bits;   fold  h_i, and whether the step acts;
//   project  w <- w - sum h_i v_i;   dots, fold  c_i, h_i <- h_i + c_i;   project  w <- w - sum c_i v_i with stage 1 of (w, w);
//   fold     beta = sqrt((w, w)); lane 0 stores T's column j and row j, beta and the count (eigsh_step);
//   normal   v_{j+1} = w / beta.
// A cycle is steps keep .. ncv - 1, the Ritz kernel (one workgroup: cyclic Jacobi on T in LDS, the order, the estimates,
// the test, Q, T <- diag(theta)) and the rotation V[:, 0:kk] <- V[:, 0:mm] Q with column mm moved to column kk.
//
// The position.  A step's column j IS a launch argument here, unlike GMRES's: start runs steps 0 .. keep - 1 and every
// cycle is the same chain, so a captured iterate(1) replays from any cycle.  A step acts when the block says that exactly
// j columns are finished, the status is RUNNING and no step met beta == 0.
//
// The freeze.  Once the status is not RUNNING every kernel that writes V, T, theta, the counts or the status returns at
// entry.  The rotation's flag is raised by a Ritz step that acts and cleared by the NEXT Ritz kernel (which is frozen or
// raises it again): the rotation has many workgroups, and none of them may clear what its siblings still read.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <memory>
#include "../../include/sblas_hip.h"
#include "capi_util.h"
#include "color.h" // the hash of the default start vector

#pragma clang fp contract(off) // file scope, ahead of the rule headers: a * b + c is two roundings everywhere below

#define EIGSH_HD __host__ __device__
#define CHEBY_HD __host__ __device__
#define GMRES_HD __host__ __device__
#include "cheby.h" // cheby_start_value
#include "eigsh.h"
#include "gmres_fold.h" // gmres_fold_sums: stage 2 of a dot, the single dot's order
#include "krylov_fold.h"

using namespace sblas;

namespace {

constexpr int G = GMRES_DOT_GROUP;
constexpr int PL = KRYLOV_PER_LANE;
constexpr int LD = EIGSH_LD;

// how a column kernel learns whether its step acts
enum { MODE_FIRST = 0,   // a step's first kernel: while the step is due
       MODE_ACTIVE = 1 };// behind a step's first fold: while ES_ACTIVE

struct ColArgs {
    int64_t n, cells, ldv;
    int nk, mode;
    const double *V;    // column i at V + i * ldv
    const double *coef; // project: h or c (device)
    double *w;
    double *part;       // dots: partial[i * cells + c]; project: stage 1 of (w, w), or NULL
    const double *blk;
};

__device__ __forceinline__ bool step_due(const long long *ib, int j)
{
    return ib[ES_STATUS] == EIGSH_RUNNING && ib[ES_COLS] == j && ib[ES_INVARIANT] == 0;
}

// nk = j + 1 columns while step j acts, else none
__device__ __forceinline__ int column_count(const double *blk, int mode, int nk)
{
    const long long *ib = reinterpret_cast<const long long *>(blk); // block-uniform loads, read once
    if (mode == MODE_FIRST) return step_due(ib, nk - 1) ? nk : 0;
    return ib[ES_ACTIVE] ? nk : 0;
}

// ---- the column walkers: gmres.hip's, restated (its device code stays what it is) -----------------------------------------
// lane t's eight elements of a cell: where they are, which exist (FULL: all), and G columns' worth of them loaded
// together so that their latencies overlap.  A group's surplus columns are clamped to the last one and never used.
template <bool FULL> struct Lane {
    int64_t first;
    bool live[PL];
    __device__ __forceinline__ Lane(int64_t n)
    {
        first = (int64_t)blockIdx.x * KRYLOV_CELL + threadIdx.x;
#pragma unroll
        for (int k = 0; k < PL; ++k) live[k] = FULL || first + k * KRYLOV_LANES < n;
    }
    __device__ __forceinline__ void load(const double *p, double (&v)[PL]) const
    {
#pragma unroll
        for (int k = 0; k < PL; ++k) v[k] = live[k] ? p[first + k * KRYLOV_LANES] : 0.0;
    }
    __device__ __forceinline__ void group(const ColArgs &a, int i0, int nk, double (&v)[G][PL]) const
    {
#pragma unroll
        for (int q = 0; q < G; ++q) {
            const int col = i0 + q < nk ? i0 + q : nk - 1;
            load(a.V + (int64_t)col * a.ldv, v[q]);
        }
    }
    __device__ __forceinline__ void store(double *p, const double (&v)[PL]) const
    {
#pragma unroll
        for (int k = 0; k < PL; ++k)
            if (live[k]) p[first + k * KRYLOV_LANES] = v[k];
    }
};

__device__ __forceinline__ bool full_cell(int64_t n) { return ((int64_t)blockIdx.x + 1) * KRYLOV_CELL <= n; }

// the multi-dot, stage 1: exactly krylov_dot_kernel's order for every column
template <bool FULL> __device__ __forceinline__ void dots_cell(const ColArgs &a, int nk, double (*ws)[4])
{
    const Lane<FULL> lane(a.n);
    double wv[PL];
    lane.load(a.w, wv);
    for (int i0 = 0; i0 < nk; i0 += G) {
        double v[G][PL];
        lane.group(a, i0, nk, v);
#pragma unroll
        for (int q = 0; q < G; ++q) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < PL; ++k)
                if (lane.live[k]) acc = acc + v[q][k] * wv[k];
            const double s = wave_fold(acc);
            if ((threadIdx.x & 63) == 0 && i0 + q < nk) ws[i0 + q][threadIdx.x >> 6] = s;
        }
    }
}

__global__ __launch_bounds__(KRYLOV_LANES) void eigsh_dots_kernel(const ColArgs a)
{
    __shared__ double ws[GMRES_MAX_DOTS][4];
    const int nk = column_count(a.blk, a.mode, a.nk);
    if (nk <= 0) return;
    if (full_cell(a.n)) dots_cell<true>(a, nk, ws); // only the last cell checks bounds
    else dots_cell<false>(a, nk, ws);
    __syncthreads();
    for (int i = threadIdx.x; i < nk; i += KRYLOV_LANES) a.part[(int64_t)i * a.cells + blockIdx.x] = (ws[i][0] + ws[i][1]) + (ws[i][2] + ws[i][3]);
}

// the projection: w <- w - coef_0 v_0 - coef_1 v_1 - ..., each product rounded and each difference rounded
template <bool FULL> __device__ __forceinline__ void project_cell(const ColArgs &a, int nk)
{
    const Lane<FULL> lane(a.n);
    double t[PL];
    lane.load(a.w, t);
    for (int i0 = 0; i0 < nk; i0 += G) {
        double v[G][PL];
        lane.group(a, i0, nk, v);
#pragma unroll
        for (int q = 0; q < G; ++q) {
            if (i0 + q < nk) { // uniform
                const double hq = a.coef[i0 + q];
#pragma unroll
                for (int k = 0; k < PL; ++k) t[k] = t[k] - hq * v[q][k];
            }
        }
    }
    lane.store(a.w, t);
    if (a.part) { // stage 1 of (w, w) over what was just written
        double acc[1] = {0.0};
#pragma unroll
        for (int k = 0; k < PL; ++k)
            if (lane.live[k]) acc[0] = acc[0] + t[k] * t[k];
        cell_store<1>(acc, a.part, a.cells);
    }
}

__global__ __launch_bounds__(KRYLOV_LANES) void eigsh_project_kernel(const ColArgs a)
{
    const int nk = column_count(a.blk, a.mode, a.nk);
    if (nk <= 0) return;
    if (full_cell(a.n)) project_cell<true>(a, nk);
    else project_cell<false>(a, nk);
}

// ---- the plan's elementwise passes -------------------------------------------------------------------------------------
// w = v0 (NULL: the hashed vector) and stage 1 of (w, w)
__global__ __launch_bounds__(KRYLOV_LANES) void eigsh_v0_kernel(int64_t n, int64_t cells, const double *v0, uint32_t salt, double *w, double *part)
{
    double acc[1] = {0.0};
    cell_walk(n, [&](int64_t i) {
        const double wi = v0 ? v0[i] : cheby_start_value(color_priority((uint32_t)i, salt));
        w[i] = wi;
        acc[0] = acc[0] + wi * wi;
    });
    cell_store<1>(acc, part, cells);
}

// v = w / beta while ES_ACTIVE, beta from the block
__global__ __launch_bounds__(KRYLOV_LANES) void eigsh_normal_kernel(int64_t n, const double *blk, const double *w, double *v)
{
    if (!reinterpret_cast<const long long *>(blk)[ES_ACTIVE]) return;
    const double beta = blk[ES_BETA];
    cell_walk(n, [&](int64_t i) { v[i] = w[i] / beta; });
}

// ---- stage 2 of the dots, and lane 0's scalar part ------------------------------------------------------------------------
enum { EF_START = 0, EF_H1, EF_H2, EF_STEP };

__global__ __launch_bounds__(KRYLOV_LANES) void eigsh_fold_kernel(int op, int j, int64_t cells, const double *part, double *blk, double *mat,
                                                                 double rtol, double atol, long long max_restarts)
{
    __shared__ double ws[GMRES_MAX_DOTS][4];
    long long *ib = reinterpret_cast<long long *>(blk);
    if (op == EF_H1) {
        if (!step_due(ib, j)) { // block-uniform, before any barrier
            if (threadIdx.x == 0) ib[ES_ACTIVE] = 0;
            return;
        }
    } else if (op != EF_START && !ib[ES_ACTIVE]) {
        return;
    }
    const int nd = op == EF_H1 || op == EF_H2 ? j + 1 : 1;
    gmres_fold_sums(nd, cells, part, cells, ws);
    if (op == EF_START && threadIdx.x < EIGSH_MAX_NCV) mat[EM_THETA + threadIdx.x] = 0.0, mat[EM_RHO + threadIdx.x] = 0.0;
    __syncthreads();
    if (threadIdx.x != 0) return;
    auto d = [&](int q) { return (ws[q][0] + ws[q][1]) + (ws[q][2] + ws[q][3]); };
    double *h = mat + EM_H, *c = mat + EM_C;
    switch (op) {
    case EF_START: {
        const double nrm = sqrt(d(0));
        const bool ok = nrm != 0.0 && isfinite(nrm);
        for (int q = 0; q < EIGSH_BLOCK_SLOTS; ++q) ib[q] = 0;
        blk[ES_BETA] = nrm, blk[ES_RTOL] = rtol, blk[ES_ATOL] = atol, ib[ES_MAX_RESTARTS] = max_restarts;
        ib[ES_STATUS] = ok ? EIGSH_RUNNING : EIGSH_BREAKDOWN, ib[ES_WHICH] = ok ? 0 : EIGSH_DENOM_V0, ib[ES_ACTIVE] = ok;
        break;
    }
    case EF_H1:
        for (int q = 0; q < nd; ++q) h[q] = d(q);
        ib[ES_ACTIVE] = 1;
        break;
    case EF_H2:
        for (int q = 0; q < nd; ++q) {
            const double cq = d(q);
            c[q] = cq, h[q] = h[q] + cq;
        }
        break;
    default:
        eigsh_step(j, h, sqrt(d(0)), mat + EM_T, blk);
        break;
    }
}

// ---- the Ritz kernel: one workgroup, T and Y in LDS ---------------------------------------------------------------------
// A round: lanes below M / 2 take the pairs' rotations from T as it stands; then every lane holds up to four 2 x 2 blocks
// in registers, all lanes have read before any writes; Y's rows take their pair's column rotation in place (a lane owns
// the two elements it rotates).  eigsh_rule.cpp's loop does the same one element after another.
__global__ __launch_bounds__(EIGSH_RITZ_THREADS) void eigsh_ritz_kernel(int k, int keep, int which, double *blk, double *mat)
{
    __shared__ double sT[LD * LD], sY[LD * LD];
    __shared__ double sc[LD / 2], ss[LD / 2], sdpp[LD / 2], sdqq[LD / 2], stheta[LD];
    __shared__ int sp[LD / 2], sq[LD / 2], sorder[LD], smet[LD], sflag[2];
    constexpr int NT = EIGSH_RITZ_THREADS;
    long long *ib = reinterpret_cast<long long *>(blk);
    const int tid = threadIdx.x;
    if (ib[ES_STATUS] != EIGSH_RUNNING) { // the freeze: only the rotation's flag falls
        if (tid == 0) ib[ES_ACT] = 0;
        return;
    }
    const int mm = (int)ib[ES_COLS];
    if (mm < 1 || mm > EIGSH_MAX_NCV) return;
    const double beta = blk[ES_BETA], rtol = blk[ES_RTOL], atol = blk[ES_ATOL];
    const long long restarts = ib[ES_RESTARTS], max_restarts = ib[ES_MAX_RESTARTS];
    const bool invariant = ib[ES_INVARIANT] != 0;
    double *T = mat + EM_T, *Y = mat + EM_Y, *theta = mat + EM_THETA, *rho = mat + EM_RHO, *Q = mat + EM_Q;
    if (tid == 0) sflag[1] = 0;
    __syncthreads();
    bool bad = false;
    for (int e = tid; e < LD * LD; e += NT) {
        const int col = e / LD, row = e % LD;
        const double v = col < mm && row < mm ? T[e] : 0.0;
        if (!isfinite(v)) bad = true;
        sT[e] = v, sY[e] = row == col && row < mm ? 1.0 : 0.0;
    }
    if (bad) sflag[1] = 1; // every writer writes the same value
    __syncthreads();
    if (sflag[1]) {
        if (tid == 0) ib[ES_STATUS] = EIGSH_BREAKDOWN, ib[ES_WHICH] = EIGSH_DENOM_T, ib[ES_ACT] = 0;
        return;
    }
    const int M = mm + (mm & 1), np = M / 2, nblocks = np * np;
    for (int sweep = 0; sweep < EIGSH_MAX_SWEEPS; ++sweep) {
        if (tid == 0) sflag[0] = 0;
        __syncthreads();
        for (int r = 0; r < M - 1; ++r) {
            if (tid < np) {
                int p, q;
                eigsh_pair(M, r, tid, &p, &q);
                double c, s, dpp, dqq;
                if (eigsh_rotation(sT[p * LD + p], sT[q * LD + q], sT[q * LD + p], &c, &s, &dpp, &dqq)) sflag[0] = 1;
                sp[tid] = p, sq[tid] = q, sc[tid] = c, ss[tid] = s, sdpp[tid] = dpp, sdqq[tid] = dqq;
            }
            __syncthreads();
            double b[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int id = tid + u * NT;
                if (id < nblocks) {
                    const int bi = id / np, bj = id - bi * np;
                    const int p1 = sp[bi], q1 = sq[bi], p2 = sp[bj], q2 = sq[bj];
                    b[u][0] = sT[p2 * LD + p1], b[u][1] = sT[q2 * LD + p1], b[u][2] = sT[p2 * LD + q1], b[u][3] = sT[q2 * LD + q1];
                    if (bi == bj) b[u][0] = sdpp[bi], b[u][3] = sdqq[bi], b[u][1] = 0.0, b[u][2] = 0.0;
                    else eigsh_block(bi < bj, sc[bi], ss[bi], sc[bj], ss[bj], &b[u][0], &b[u][1], &b[u][2], &b[u][3]);
                }
            }
            for (int it = tid; it < mm * np; it += NT) {
                const int i = it / mm, row = it - i * mm;
                eigsh_rotate_pair(sc[i], ss[i], &sY[sp[i] * LD + row], &sY[sq[i] * LD + row]);
            }
            __syncthreads(); // every block is read
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int id = tid + u * NT;
                if (id < nblocks) {
                    const int bi = id / np, bj = id - bi * np;
                    const int p1 = sp[bi], q1 = sq[bi], p2 = sp[bj], q2 = sq[bj];
                    sT[p2 * LD + p1] = b[u][0], sT[q2 * LD + p1] = b[u][1], sT[p2 * LD + q1] = b[u][2], sT[q2 * LD + q1] = b[u][3];
                }
            }
            __syncthreads();
        }
        const int rotated = sflag[0];
        __syncthreads();
        if (!rotated) break;
    }
    // the order: rank i = how many come before it (the identity first: values that do not order, a NaN from an overflow,
    // must leave no entry unwritten)
    if (tid < LD) sorder[tid] = tid;
    __syncthreads();
    if (tid < mm) {
        int rank = 0;
        for (int j = 0; j < mm; ++j)
            if (j != tid && eigsh_before(which, sT[j * LD + j], j, sT[tid * LD + tid], tid)) ++rank;
        sorder[rank] = tid;
    }
    __syncthreads();
    const int kk = keep < mm ? keep : mm;
    if (tid < mm) {
        const int i = sorder[tid];
        const double th = sT[i * LD + i], est = fabs(beta * sY[i * LD + (mm - 1)]);
        stheta[tid] = th, theta[tid] = th, rho[tid] = est;
        smet[tid] = tid < k && eigsh_met(est, th, rtol, atol);
    }
    for (int e = tid; e < kk * mm; e += NT) {
        const int r = e / mm, l = e - r * mm;
        Q[r * LD + l] = sY[sorder[r] * LD + l];
    }
    for (int e = tid; e < LD * LD; e += NT) Y[e] = sY[e];
    __syncthreads();
    for (int e = tid; e < LD * LD; e += NT) {
        const int col = e / LD, row = e % LD;
        T[e] = row == col && row < kk ? stheta[row] : 0.0;
    }
    if (tid != 0) return;
    int met = 0;
    for (int r = 0; r < mm && r < k; ++r) met += smet[r];
    int64_t which_out = 0;
    const int st = eigsh_decide(mm, k, met, invariant, (int64_t)restarts + 1, (int64_t)max_restarts, &which_out);
    ib[ES_RESTARTS] = restarts + 1, ib[ES_STATUS] = st, ib[ES_WHICH] = which_out, ib[ES_CONVERGED] = met;
    ib[ES_COLS] = kk, ib[ES_MM] = mm, ib[ES_KK] = kk, ib[ES_ACT] = 1;
}

// ---- the rotation: V[:, 0:kk] <- V[:, 0:mm] Q in place, column mm to column kk ------------------------------------------------
// A lane owns one row of V: its mm values wait in registers (MM is the tier, so no index is a run-time one and nothing
// goes to scratch), every column load is coalesced, Q is read from LDS at an address all lanes share.  The order is
// gmres_combine's: the first product copied, then rounded product and rounded sum ascending.
struct RotArgs {
    int64_t n, ldv;
    double *V;
    const double *Q;
    int ldq, mm, kk;
    const double *blk; // the plan's: act, mm and kk come from the block
};

template <int MM> __global__ __launch_bounds__(EIGSH_ROTATE_THREADS) void eigsh_rotate_kernel(const RotArgs a)
{
    __shared__ double sQ[MM * MM];
    int mm = a.mm, kk = a.kk;
    if (a.blk) {
        const long long *ib = reinterpret_cast<const long long *>(a.blk);
        if (!ib[ES_ACT]) return;
        mm = (int)ib[ES_MM], kk = (int)ib[ES_KK];
    }
    if (mm < 1 || mm > MM || kk < 1 || kk > mm) return;
    for (int e = threadIdx.x; e < kk * mm; e += EIGSH_ROTATE_THREADS) {
        const int i = e / mm, l = e - i * mm;
        sQ[i * MM + l] = a.Q[(int64_t)i * a.ldq + l];
    }
    __syncthreads();
    const int64_t row = (int64_t)blockIdx.x * EIGSH_ROTATE_THREADS + threadIdx.x;
    if (row >= a.n) return;
    double *p = a.V + row;
    double v[MM];
#pragma unroll
    for (int l = 0; l < MM; ++l) v[l] = l < mm ? p[(int64_t)l * a.ldv] : 0.0;
    const double last = p[(int64_t)mm * a.ldv];
    for (int i = 0; i < kk; ++i) {
        const double *q = sQ + i * MM;
        double acc = q[0] * v[0];
#pragma unroll
        for (int l = 1; l < MM; ++l)
            if (l < mm) acc = acc + q[l] * v[l];
        p[(int64_t)i * a.ldv] = acc;
    }
    p[(int64_t)kk * a.ldv] = last;
}

void launch_rotate(hipStream_t s, int tier_mm, const RotArgs &a)
{
    const unsigned grid = (unsigned)((a.n + EIGSH_ROTATE_THREADS - 1) / EIGSH_ROTATE_THREADS);
    if (tier_mm <= 8) eigsh_rotate_kernel<8><<<grid, EIGSH_ROTATE_THREADS, 0, s>>>(a);
    else if (tier_mm <= 16) eigsh_rotate_kernel<16><<<grid, EIGSH_ROTATE_THREADS, 0, s>>>(a);
    else if (tier_mm <= 32) eigsh_rotate_kernel<32><<<grid, EIGSH_ROTATE_THREADS, 0, s>>>(a);
    else eigsh_rotate_kernel<64><<<grid, EIGSH_ROTATE_THREADS, 0, s>>>(a);
}

// ---- the plan ------------------------------------------------------------------------------------------------------------
struct EigshPlan {
    int dev = -1, k = 0, ncv = 0, keep = 0, which = 0;
    uint32_t seed = 0;
    int64_t n = 0, nnz = 0, cells = 0, ldv = 0;
    const int32_t *rowptr = nullptr, *colidx = nullptr; // the caller's
    const void *spmv = nullptr;
    size_t vector_bytes = 0, partial_bytes = 0, bytes = 0;
    DeviceBuffer buf; // block | small matrices | partials | V (ncv + 1 columns), w
    double *blk = nullptr, *mat = nullptr, *part = nullptr, *vec = nullptr;
    bool started = false;
    const double *val = nullptr;
    double *col(int j) const { return vec + (size_t)j * (size_t)ldv; }
    double *w() const { return col(ncv + 1); }
};

void fold(const EigshPlan *p, hipStream_t s, int op, int j, double rtol = 0.0, double atol = 0.0, int64_t max_restarts = 0)
{
    eigsh_fold_kernel<<<1, KRYLOV_LANES, 0, s>>>(op, j, p->cells, p->part, p->blk, p->mat, rtol, atol, (long long)max_restarts);
}

// y = A x: through the SpMV plan where one was given (precond.h's plan_spmv, restated: this plan has no preconditioner)
int spmv(const EigshPlan *p, hipStream_t s, const double *x, double *y)
{
    if (p->spmv)
        return sblas_hip_spmv_csr_f64_i32_planned(p->spmv, -1, s, p->n, p->n, p->nnz, p->rowptr, p->colidx, p->val, x, 1.0, 0.0, y);
    return sblas_hip_spmv_csr_f64_i32(-1, s, p->n, p->n, p->nnz, p->rowptr, p->colidx, p->val, x, 1.0, 0.0, y);
}

int step_launches(const EigshPlan *p, hipStream_t s, int j)
{
    const unsigned grid = (unsigned)p->cells;
    const int rc = spmv(p, s, p->col(j), p->w());
    if (rc != SBLAS_OK) return rc;
    auto cols = [&](int mode, const double *coef, double *part) { return ColArgs{p->n, p->cells, p->ldv, j + 1, mode, p->vec, coef, p->w(), part, p->blk}; };
    eigsh_dots_kernel<<<grid, KRYLOV_LANES, 0, s>>>(cols(MODE_FIRST, nullptr, p->part));
    fold(p, s, EF_H1, j);
    eigsh_project_kernel<<<grid, KRYLOV_LANES, 0, s>>>(cols(MODE_ACTIVE, p->mat + EM_H, nullptr));
    eigsh_dots_kernel<<<grid, KRYLOV_LANES, 0, s>>>(cols(MODE_ACTIVE, nullptr, p->part));
    fold(p, s, EF_H2, j);
    eigsh_project_kernel<<<grid, KRYLOV_LANES, 0, s>>>(cols(MODE_ACTIVE, p->mat + EM_C, p->part));
    fold(p, s, EF_STEP, j);
    eigsh_normal_kernel<<<grid, KRYLOV_LANES, 0, s>>>(p->n, p->blk, p->w(), p->col(j + 1));
    return SBLAS_OK;
}

bool current(const EigshPlan *p) { return p && p->dev == resolve_device(-1); }

} // namespace

extern "C" {

int sblas_hip_eigsh_rotate_f64(int dev, void *stream, int64_t n, int mm, int keep, double *V, int64_t ldv, const double *Q, int ldq)
{
    if (n < 0 || n > INT_MAX || mm < 1 || mm > EIGSH_MAX_NCV || keep < 1 || keep > mm || ldv < n || ldq < mm || !Q || (n > 0 && !V))
        return SBLAS_E_INVALID;
    if (n == 0) return SBLAS_OK;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    launch_rotate((hipStream_t)stream, mm, RotArgs{n, ldv, V, Q, ldq, mm, keep, nullptr});
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_eigsh_ritz_f64(int dev, void *stream, int k, int keep, int which, double *blk, double *mat)
{
    if (!blk || !mat || !eigsh_which_ok(which) || k < 1 || keep < k || keep > EIGSH_MAX_NCV - 1) return SBLAS_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(blk) | reinterpret_cast<uintptr_t>(mat)) & 7u) return SBLAS_E_INVALID;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    eigsh_ritz_kernel<<<1, EIGSH_RITZ_THREADS, 0, (hipStream_t)stream>>>(k, keep, which, blk, mat);
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_eigsh_plan_create(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx, int k, int ncv,
                                int keep, int which, const void *spmv_plan, uint32_t seed, void **plan_out)
{
    if (!plan_out) return SBLAS_E_INVALID;
    *plan_out = nullptr;
    if (n < 0 || nnz < 0 || n > INT_MAX - 64 || nnz > INT_MAX || !rowptr || (nnz > 0 && !colidx)) return SBLAS_E_INVALID;
    int64_t sizes[2];
    if (!eigsh_which_ok(which) || sblas_eigsh_sizes(n, k, ncv, keep, sizes) != SBLAS_OK) return SBLAS_E_INVALID;
    const int device = resolve_device(dev);
    if (spmv_plan && sblas_hip_spmv_plan_speaks_for(spmv_plan, device, n, n, nnz, rowptr, colidx) != SBLAS_OK) return SBLAS_E_INVALID;
    std::unique_ptr<EigshPlan> p(new EigshPlan);
    p->dev = device, p->k = k, p->ncv = (int)sizes[0], p->keep = (int)sizes[1], p->which = which, p->seed = seed;
    p->n = n, p->nnz = nnz, p->cells = krylov_cells(n), p->rowptr = rowptr, p->colidx = colidx, p->spmv = spmv_plan;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    const size_t block_bytes = pad256(EIGSH_BLOCK_SLOTS * 8), matrix_bytes = pad256((size_t)EIGSH_MATRIX_DOUBLES * 8);
    p->vector_bytes = pad256((size_t)n * 8), p->ldv = (int64_t)(p->vector_bytes / 8);
    p->partial_bytes = pad256((size_t)p->ncv * (size_t)p->cells * 8);
    p->bytes = block_bytes + matrix_bytes + p->partial_bytes + (size_t)(p->ncv + 2) * p->vector_bytes;
    if (p->buf.alloc(p->dev, p->bytes) != hipSuccess) return SBLAS_E_HIP;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(p->buf.at<char>(), 0, p->bytes, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return SBLAS_E_HIP;
    p->blk = p->buf.at<double>(), p->mat = p->buf.at<double>(block_bytes), p->part = p->buf.at<double>(block_bytes + matrix_bytes);
    p->vec = p->buf.at<double>(block_bytes + matrix_bytes + p->partial_bytes);
    *plan_out = p.release();
    return SBLAS_OK;
}

int sblas_hip_eigsh_info(const void *plan, int64_t out[14])
{
    if (!plan || !out) return SBLAS_E_INVALID;
    const EigshPlan *p = static_cast<const EigshPlan *>(plan);
    int64_t launches[4] = {0};
    sblas_eigsh_launches(p->ncv, p->keep, launches);
    out[0] = p->n, out[1] = p->nnz, out[2] = p->k, out[3] = p->ncv, out[4] = p->keep, out[5] = p->which, out[6] = (int64_t)p->vector_bytes;
    out[7] = (int64_t)p->partial_bytes, out[8] = EIGSH_BLOCK_SLOTS * 8, out[9] = (int64_t)EIGSH_MATRIX_DOUBLES * 8, out[10] = (int64_t)p->bytes;
    out[11] = launches[0], out[12] = launches[1], out[13] = launches[2];
    return SBLAS_OK;
}

int sblas_hip_eigsh_destroy(void *plan)
{
    delete static_cast<EigshPlan *>(plan);
    return SBLAS_OK;
}

int sblas_hip_eigsh_start(void *plan, void *stream, const double *val, const double *v0, double rtol, double atol, int64_t max_restarts)
{
    EigshPlan *p = static_cast<EigshPlan *>(plan);
    if (!current(p)) return SBLAS_E_INVALID;
    if (!(rtol >= 0.0) || !(atol >= 0.0) || max_restarts < 0 || (p->nnz > 0 && !val)) return SBLAS_E_INVALID; // a NaN tolerance is refused too
    p->started = false, p->val = val;
    hipStream_t s = (hipStream_t)stream;
    const unsigned grid = (unsigned)p->cells;
    eigsh_v0_kernel<<<grid, KRYLOV_LANES, 0, s>>>(p->n, p->cells, v0, color_salt(p->seed), p->w(), p->part);
    fold(p, s, EF_START, 0, rtol, atol, max_restarts);
    eigsh_normal_kernel<<<grid, KRYLOV_LANES, 0, s>>>(p->n, p->blk, p->w(), p->col(0));
    for (int j = 0; j < p->keep; ++j) {
        const int rc = step_launches(p, s, j);
        if (rc != SBLAS_OK) return rc;
    }
    if (hipGetLastError() != hipSuccess) return SBLAS_E_HIP;
    p->started = true;
    return SBLAS_OK;
}

int sblas_hip_eigsh_iterate(void *plan, void *stream, int64_t cycles)
{
    EigshPlan *p = static_cast<EigshPlan *>(plan);
    if (!current(p) || cycles < 0 || !p->started) return SBLAS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    for (int64_t it = 0; it < cycles; ++it) {
        for (int j = p->keep; j < p->ncv; ++j) {
            const int rc = step_launches(p, s, j);
            if (rc != SBLAS_OK) return rc;
        }
        eigsh_ritz_kernel<<<1, EIGSH_RITZ_THREADS, 0, s>>>(p->k, p->keep, p->which, p->blk, p->mat);
        launch_rotate(s, p->ncv, RotArgs{p->n, p->ldv, p->vec, p->mat + EM_Q, LD, 0, 0, p->blk});
    }
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_eigsh_status(const void *plan, void *stream, double out[8], double *theta, double *residuals)
{
    const EigshPlan *p = static_cast<const EigshPlan *>(plan);
    if (!current(p) || !out || !p->started) return SBLAS_E_INVALID;
    double h[EIGSH_BLOCK_SLOTS];
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(h, p->blk, sizeof h, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && theta) e = hipMemcpyAsync(theta, p->mat + EM_THETA, (size_t)p->k * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && residuals) e = hipMemcpyAsync(residuals, p->mat + EM_RHO, (size_t)p->k * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return SBLAS_E_HIP;
    long long ih[EIGSH_BLOCK_SLOTS];
    memcpy(ih, h, sizeof ih);
    out[0] = (double)ih[ES_STATUS], out[1] = (double)ih[ES_RESTARTS], out[2] = (double)ih[ES_MATVECS], out[3] = (double)ih[ES_CONVERGED];
    out[4] = h[ES_BETA], out[5] = (double)ih[ES_WHICH], out[6] = (double)ih[ES_MM], out[7] = (double)ih[ES_COLS];
    return SBLAS_OK;
}

int sblas_hip_eigsh_values(const void *plan, void *stream, double *out)
{
    const EigshPlan *p = static_cast<const EigshPlan *>(plan);
    if (!current(p) || !out || !p->started) return SBLAS_E_INVALID;
    const hipError_t e = hipMemcpyAsync(out, p->mat + EM_THETA, (size_t)p->k * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    return e == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_eigsh_vectors(const void *plan, const double **V, int64_t *ldv)
{
    const EigshPlan *p = static_cast<const EigshPlan *>(plan);
    if (!p || !V || !ldv) return SBLAS_E_INVALID;
    *V = p->vec, *ldv = p->ldv;
    return SBLAS_OK;
}

} // extern "C"
