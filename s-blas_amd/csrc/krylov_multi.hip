// krylov_multi.hip -- PCG and BiCGStab for s right-hand sides at once: s independent recurrences that
// share A and run in lockstep, one SpMM per product instead of s SpMVs.  X, B and the work blocks are n x s row-major.
// Everything between two SpMMs is one of krylov.hip's three kernels, widened by a column tile:
//   dot     stage 1 of up to KRYLOV_MAX_DOTS dots of every column in one pass: one workgroup a cell of KRYLOV_CELL rows
//           and a tile of TILE columns (tile.h), a lane its row's eight doubles of each operand and one accumulator
//           per column and dot; the sum of dot k, column j, cell c to part[(k * s + j) * cells + c];
//   update  the fused updates of krylov.hip with column j's own alpha, beta, omega from scalar block j, also stage 1 of
//           the dots of what they wrote;
//   fold    stage 2: one workgroup PER COLUMN folds that column's cells and its lane 0 takes the scalar step on block j
//           (krylov_scalar.h: the text krylov.hip runs).
// A column's dot walks its rows exactly as krylov.hip's dot walks a vector (cell_walk's order, the same butterfly), so
// it has the pinned dot's bits on the strided column.  Nothing waits across workgroups: no flag polling, no cooperative
// launch, no atomics.  The host passes no scalar of the recurrence.
//
// The freeze, per column.  A tile reads its columns' status words once (uniform loads) into a mask.  A tile whose
// columns are all frozen returns at entry; a mixed tile predicates every load and store by the mask, so a frozen column
// of any vector is neither read nor written; lane 0 of a frozen column's fold changes nothing.  The SpMM still
// multiplies the frozen columns of the direction block, into work blocks only.
//
// Width of the accesses.  A full tile whose columns all run moves a row's eight doubles as four 16-byte accesses when
// every base and leading dimension of the launch is a multiple of 16 bytes (decided on the host, a template flag);
// anything else -- the ragged last tile, a mixed tile, an odd leading dimension, a base offset by one element -- goes
// double by double.  Same values, same order, same bits.
//
// An applied preconditioner: a plan seated through create_ex -- the AMG block cycle -- or a pair of
// solve plans seated through create_pair -- ILU(0), the two tiled solves with the second in place -- runs between the
// solver's kernels where krylov.hip applies M^-1: PCG on R into Z, then the dots (r, z) and the fold that takes rho or
// beta; BiCGStab on P into P^ and on S into S^.  It runs on ALL columns, into work blocks only and never into X: a
// frozen column's operand no longer changes, so its result is recomputed to the same bits, and no column of the cycle
// can reach another column.
//
// Arithmetic.  Contraction is off at file scope, as in krylov.hip: every product and every sum is rounded on its own.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <string.h>
#include <initializer_list>
#include <memory>
#include <type_traits>
#include "../../include/sblas_hip.h"
#include "capi_util.h"
#include "krylov.h"
#include "krylov_multi.h"
#include "multi_plan.h" // the plan base: bind, layout, product, the refusals of start, status
#include "unit_row.h"   // tile_ld, tile_st, tile_id

#pragma clang fp contract(off) // file scope: a * b + c below is two roundings on every path

#include "krylov_fold.h"   // wave_fold, group_fold, cells_fold
#include "krylov_scalar.h" // the fold ops and the scalar step
#include "krylov_tile.h"   // row_walk, tile_store

using namespace sblas;

namespace {

constexpr int T = TILE;
// internal update ops, after the public SBLAS_KRYLOV_UP_* ones (krylov.hip's)
enum { UP_COPY = 5, UP_START_PCG = 6, UP_START_BICG = 7 };

struct MUpArgs {
    int64_t n, cells;
    int s;
    double *blk;  // s scalar blocks
    double *part; // dot k, column j, cell c at part[(k * s + j) * cells + c]
    double *v[8];
    int64_t ld[8]; // of v[q]; a dinv vector's is not read
};

struct MDotArgs {
    int64_t n, cells;
    int s;
    const double *x[KRYLOV_MAX_DOTS], *y[KRYLOV_MAX_DOTS];
    int64_t ldx[KRYLOV_MAX_DOTS], ldy[KRYLOV_MAX_DOTS];
    double *part;
};

// ---- dot, stage 1 ----------------------------------------------------------------------------------------------------
// not a part of the freeze: like krylov.hip's dot it reads work blocks (or the caller's operands) and writes partials
template <int ND, bool WIDE> __global__ __launch_bounds__(KRYLOV_LANES) void multi_dot_kernel(const MDotArgs a)
{
    const TileId id = tile_id(a.cells, tiles(a.s));
    const int j0 = (int)id.tile * T, w = a.s - j0 < T ? a.s - j0 : T;
    const unsigned mask = (1u << w) - 1u;
    double acc[ND * T];
#pragma unroll
    for (int q = 0; q < ND * T; ++q) acc[q] = 0.0;
    auto body = [&](auto fast) {
        constexpr bool F = decltype(fast)::value;
        row_walk(id.block, a.n, [&](int64_t i) {
#pragma unroll
            for (int q = 0; q < ND; ++q) {
                double x[T], y[T];
                tile_ld<T, F>(a.x[q] + i * a.ldx[q] + j0, mask, x);
                tile_ld<T, F>(a.y[q] + i * a.ldy[q] + j0, mask, y);
#pragma unroll
                for (int c = 0; c < T; ++c) acc[q * T + c] = acc[q * T + c] + x[c] * y[c];
            }
        });
    };
    if (WIDE && w == T) body(std::true_type{});
    else body(std::false_type{});
    tile_store<ND>(acc, a.part, a.s, a.cells, id.block, j0, mask);
}

// ---- the fused updates -----------------------------------------------------------------------------------------------
// krylov.hip's updates on eight columns of a row, column c with its own scalars.  JAC: dinv[i] is read once per row.
// Blocks are not __restrict__: without a preconditioner Z is R, and P^, S^ are P, S.
template <int OP, bool JAC, bool WIDE> __global__ __launch_bounds__(KRYLOV_LANES) void multi_update_kernel(const MUpArgs a)
{
    constexpr bool START = OP == UP_START_PCG || OP == UP_START_BICG;
    const TileId id = tile_id(a.cells, tiles(a.s));
    const int j0 = (int)id.tile * T, w = a.s - j0 < T ? a.s - j0 : T;
    unsigned mask = 0, zmask = 0; // the columns that run; of a start pass, those with b == 0
    double al[T], be[T], om[T];
#pragma unroll
    for (int c = 0; c < T; ++c) {
        al[c] = be[c] = om[c] = 0.0;
        if (c < w) { // block-uniform, read once: the freeze
            const double *b = a.blk + (size_t)(j0 + c) * KRYLOV_BLOCK_SLOTS;
            const long long *ib = reinterpret_cast<const long long *>(b);
            if (START || ib[KS_STATUS] == SBLAS_KRYLOV_RUNNING) mask |= 1u << c;
            if (START && ib[KS_ZERO_X] != 0) zmask |= 1u << c;
            if (!START) al[c] = b[KS_ALPHA], be[c] = b[KS_BETA], om[c] = b[KS_OMEGA];
        }
    }
    if (mask == 0) return; // every column of the tile is frozen
    double *const *v = a.v;
    const int64_t *ld = a.ld;
    constexpr int NP = (OP == SBLAS_KRYLOV_UP_PCG_XR || OP == UP_START_PCG) ? (JAC ? 2 : 1) : OP == SBLAS_KRYLOV_UP_BICG_XR ? 2 : OP == UP_START_BICG ? 1 : 0;
    double acc[(NP ? NP : 1) * T];
#pragma unroll
    for (int q = 0; q < (NP ? NP : 1) * T; ++q) acc[q] = 0.0;
    auto at = [&](int q, int64_t i) { return v[q] + i * ld[q] + j0; };
    auto body = [&](auto fast) {
        constexpr bool F = decltype(fast)::value;
        row_walk(id.block, a.n, [&](int64_t i) {
            if constexpr (OP == SBLAS_KRYLOV_UP_PCG_XR) { // x, r, p, q, dinv, z
                double x[T], p[T], r[T], q[T];
                tile_ld<T, F>(at(0, i), mask, x), tile_ld<T, F>(at(2, i), mask, p);
#pragma unroll
                for (int c = 0; c < T; ++c) x[c] = x[c] + al[c] * p[c];
                tile_st<T, F>(at(0, i), mask, x);
                tile_ld<T, F>(at(1, i), mask, r), tile_ld<T, F>(at(3, i), mask, q);
#pragma unroll
                for (int c = 0; c < T; ++c) {
                    r[c] = r[c] - al[c] * q[c];
                    acc[c] = acc[c] + r[c] * r[c];
                }
                tile_st<T, F>(at(1, i), mask, r);
                if constexpr (JAC) {
                    const double di = v[4][i];
                    double z[T];
#pragma unroll
                    for (int c = 0; c < T; ++c) {
                        z[c] = di * r[c];
                        acc[T + c] = acc[T + c] + r[c] * z[c];
                    }
                    tile_st<T, F>(at(5, i), mask, z);
                }
            } else if constexpr (OP == SBLAS_KRYLOV_UP_PCG_P) { // p, z
                double p[T], z[T];
                tile_ld<T, F>(at(0, i), mask, p), tile_ld<T, F>(at(1, i), mask, z);
#pragma unroll
                for (int c = 0; c < T; ++c) p[c] = z[c] + be[c] * p[c];
                tile_st<T, F>(at(0, i), mask, p);
            } else if constexpr (OP == UP_COPY) { // dst, src
                double x[T];
                tile_ld<T, F>(at(1, i), mask, x);
                tile_st<T, F>(at(0, i), mask, x);
            } else if constexpr (OP == SBLAS_KRYLOV_UP_BICG_P) { // p, r, v, dinv, p^
                double p[T], r[T], vv[T];
                tile_ld<T, F>(at(0, i), mask, p), tile_ld<T, F>(at(1, i), mask, r), tile_ld<T, F>(at(2, i), mask, vv);
#pragma unroll
                for (int c = 0; c < T; ++c) p[c] = r[c] + be[c] * (p[c] - om[c] * vv[c]);
                tile_st<T, F>(at(0, i), mask, p);
                if constexpr (JAC) {
                    const double di = v[3][i];
#pragma unroll
                    for (int c = 0; c < T; ++c) p[c] = di * p[c];
                    tile_st<T, F>(at(4, i), mask, p);
                }
            } else if constexpr (OP == SBLAS_KRYLOV_UP_BICG_S) { // s, r, v, dinv, s^
                double sv[T], r[T], vv[T];
                tile_ld<T, F>(at(1, i), mask, r), tile_ld<T, F>(at(2, i), mask, vv);
#pragma unroll
                for (int c = 0; c < T; ++c) sv[c] = r[c] - al[c] * vv[c];
                tile_st<T, F>(at(0, i), mask, sv);
                if constexpr (JAC) {
                    const double di = v[3][i];
#pragma unroll
                    for (int c = 0; c < T; ++c) sv[c] = di * sv[c];
                    tile_st<T, F>(at(4, i), mask, sv);
                }
            } else if constexpr (OP == SBLAS_KRYLOV_UP_BICG_XR) { // x, r, p^, s^, s, t, r^
                double x[T], ph[T], sh[T];
                tile_ld<T, F>(at(0, i), mask, x), tile_ld<T, F>(at(2, i), mask, ph), tile_ld<T, F>(at(3, i), mask, sh);
#pragma unroll
                for (int c = 0; c < T; ++c) x[c] = (x[c] + al[c] * ph[c]) + om[c] * sh[c];
                tile_st<T, F>(at(0, i), mask, x);
                double sv[T], t[T], rh[T];
                tile_ld<T, F>(at(4, i), mask, sv), tile_ld<T, F>(at(5, i), mask, t), tile_ld<T, F>(at(6, i), mask, rh);
#pragma unroll
                for (int c = 0; c < T; ++c) {
                    sv[c] = sv[c] - om[c] * t[c];
                    acc[c] = acc[c] + sv[c] * sv[c];
                    acc[T + c] = acc[T + c] + rh[c] * sv[c];
                }
                tile_st<T, F>(at(1, i), mask, sv);
            } else if constexpr (OP == UP_START_PCG) { // r, b, q (= A x0), dinv, z, x
                double b[T], q[T], r[T];
                tile_ld<T, F>(at(1, i), mask, b), tile_ld<T, F>(at(2, i), mask, q);
                double *x = at(5, i);
#pragma unroll
                for (int c = 0; c < T; ++c) {
                    const bool zero = zmask >> c & 1u; // b == 0: x = 0, and b - A x0 is not formed
                    if (zero) x[c] = 0.0;
                    r[c] = zero ? 0.0 : b[c] - q[c];
                    acc[c] = acc[c] + r[c] * r[c];
                }
                tile_st<T, F>(at(0, i), mask, r);
                if constexpr (JAC) {
                    const double di = v[3][i];
                    double z[T];
#pragma unroll
                    for (int c = 0; c < T; ++c) {
                        z[c] = (zmask >> c & 1u) ? 0.0 : di * r[c];
                        acc[T + c] = acc[T + c] + r[c] * z[c];
                    }
                    tile_st<T, F>(at(4, i), mask, z);
                }
            } else { // UP_START_BICG: r, b, v (= A x0 on entry, 0 on exit), r^, p, x
                double b[T], q[T], r[T], zero8[T];
                tile_ld<T, F>(at(1, i), mask, b), tile_ld<T, F>(at(2, i), mask, q);
                double *x = at(5, i);
#pragma unroll
                for (int c = 0; c < T; ++c) {
                    const bool zero = zmask >> c & 1u;
                    if (zero) x[c] = 0.0;
                    r[c] = zero ? 0.0 : b[c] - q[c];
                    zero8[c] = 0.0;
                    acc[c] = acc[c] + r[c] * r[c];
                }
                tile_st<T, F>(at(0, i), mask, r), tile_st<T, F>(at(3, i), mask, r);
                tile_st<T, F>(at(4, i), mask, zero8), tile_st<T, F>(at(2, i), mask, zero8);
            }
        });
    };
    if (WIDE && mask == (1u << T) - 1u) body(std::true_type{});
    else body(std::false_type{});
    if constexpr (NP > 0) tile_store<NP>(acc, a.part, a.s, a.cells, id.block, j0, mask);
}

// ---- stage 2, which is also the scalar step: one workgroup a column -------------------------------------------------------
__global__ __launch_bounds__(KRYLOV_LANES) void multi_fold_kernel(int op, int nd, int flag, int s, int64_t cells, const double *part, double *blk,
                                                                 double *out, double rtol, double atol, long long max_iter)
{
    const int j = (int)blockIdx.x;
    double d[KRYLOV_MAX_DOTS];
    cells_fold(nd, cells, part + (int64_t)j * cells, (int64_t)s * cells, d); // krylov.hip's lane walk over column j's cells
    if (threadIdx.x != 0) return;
    if (op == FOLD_OUT) {
        for (int q = 0; q < nd; ++q) out[(int64_t)q * s + j] = d[q];
        return;
    }
    krylov_scalar_step(op, nd, flag, d, blk + (size_t)j * KRYLOV_BLOCK_SLOTS, rtol, atol, max_iter);
}

// ---- launches ----------------------------------------------------------------------------------------------------------
template <int ND> inline void launch_dot_nd(hipStream_t st, bool wide, const MDotArgs &a)
{
    if (wide) multi_dot_kernel<ND, true><<<(unsigned)tile_grid(a.cells, a.s), KRYLOV_LANES, 0, st>>>(a);
    else multi_dot_kernel<ND, false><<<(unsigned)tile_grid(a.cells, a.s), KRYLOV_LANES, 0, st>>>(a);
}

inline void launch_dot(hipStream_t st, int nd, const MDotArgs &a)
{
    bool wide = true;
    for (int q = 0; q < nd; ++q) wide = wide && wide16(a.x[q], a.ldx[q]) && wide16(a.y[q], a.ldy[q]);
    if (nd == 1) launch_dot_nd<1>(st, wide, a);
    else if (nd == 2) launch_dot_nd<2>(st, wide, a);
    else launch_dot_nd<3>(st, wide, a);
}

inline void launch_fold(hipStream_t st, int op, int nd, int flag, int s, int64_t cells, const double *part, double *blk, double *out = nullptr,
                        double rtol = 0.0, double atol = 0.0, int64_t max_iter = 0)
{
    multi_fold_kernel<<<(unsigned)s, KRYLOV_LANES, 0, st>>>(op, nd, flag, s, cells, part, blk, out, rtol, atol, (long long)max_iter);
}

template <int OP, bool JAC> inline void launch_update_op(hipStream_t st, bool wide, const MUpArgs &a)
{
    if (wide) multi_update_kernel<OP, JAC, true><<<(unsigned)tile_grid(a.cells, a.s), KRYLOV_LANES, 0, st>>>(a);
    else multi_update_kernel<OP, JAC, false><<<(unsigned)tile_grid(a.cells, a.s), KRYLOV_LANES, 0, st>>>(a);
}

// blocks of an op (the single update's counts) and the place of dinv among them with Jacobi, else -1
const int NEED[8] = {4, 2, 3, 3, 7, 2, 3, 6};
inline int dinv_place(int op, bool jac)
{
    if (!jac) return -1;
    return op == SBLAS_KRYLOV_UP_PCG_XR ? 4 : op == SBLAS_KRYLOV_UP_BICG_P || op == SBLAS_KRYLOV_UP_BICG_S || op == UP_START_PCG ? 3 : -1;
}
inline int blocks_of(int op, bool jac)
{
    if (op == UP_START_PCG) return 6; // r, b, q, dinv, z, x: x is the last, with or without Jacobi
    return NEED[op] + (dinv_place(op, jac) >= 0 ? 2 : 0);
}

inline void launch_update(hipStream_t st, int op, bool jac, const MUpArgs &a)
{
    jac = dinv_place(op, jac) >= 0;
    const int nv = blocks_of(op, jac), dp = dinv_place(op, jac);
    bool wide = true;
    for (int q = 0; q < nv; ++q)
        if (q != dp && a.v[q]) wide = wide && wide16(a.v[q], a.ld[q]);
    switch (op) {
    case SBLAS_KRYLOV_UP_PCG_XR: return jac ? launch_update_op<SBLAS_KRYLOV_UP_PCG_XR, true>(st, wide, a) : launch_update_op<SBLAS_KRYLOV_UP_PCG_XR, false>(st, wide, a);
    case SBLAS_KRYLOV_UP_PCG_P: return launch_update_op<SBLAS_KRYLOV_UP_PCG_P, false>(st, wide, a);
    case SBLAS_KRYLOV_UP_BICG_P: return jac ? launch_update_op<SBLAS_KRYLOV_UP_BICG_P, true>(st, wide, a) : launch_update_op<SBLAS_KRYLOV_UP_BICG_P, false>(st, wide, a);
    case SBLAS_KRYLOV_UP_BICG_S: return jac ? launch_update_op<SBLAS_KRYLOV_UP_BICG_S, true>(st, wide, a) : launch_update_op<SBLAS_KRYLOV_UP_BICG_S, false>(st, wide, a);
    case SBLAS_KRYLOV_UP_BICG_XR: return launch_update_op<SBLAS_KRYLOV_UP_BICG_XR, false>(st, wide, a);
    case UP_COPY: return launch_update_op<UP_COPY, false>(st, wide, a);
    case UP_START_PCG: return jac ? launch_update_op<UP_START_PCG, true>(st, wide, a) : launch_update_op<UP_START_PCG, false>(st, wide, a);
    default: return launch_update_op<UP_START_BICG, false>(st, wide, a);
    }
}

// ---- the plan ----------------------------------------------------------------------------------------------------------
struct MultiPlan : MultiPlanBase { // scalar blocks | partials | the SpMM's workspace | work blocks
    int method = 0;
    double *w(int k) const { return vec + (size_t)k * (block_bytes / 8); }
    const double *dinv() const { return pre.jacobi() ? pre.values : nullptr; } // the kernels', NULL unless the kind is Jacobi
};

// work blocks of the plan, by slot (krylov.hip's)
enum { V_R = 0, V_P = 1, V_Q = 2, V_Z = 3 };
enum { B_R = 0, B_RHAT = 1, B_P = 2, B_V = 3, B_S = 4, B_T = 5, B_PH = 6, B_SH = 7 };

struct Blk {
    double *p;
    int64_t ld;
};

MUpArgs up_args(const MultiPlan *p, std::initializer_list<Blk> v)
{
    MUpArgs a{p->n, p->cells, p->s, p->blk, p->part, {}, {}};
    int k = 0;
    for (const Blk &q : v) a.v[k] = q.p, a.ld[k] = q.ld, ++k;
    return a;
}

void dot(const MultiPlan *p, hipStream_t st, Blk x0, Blk y0, Blk x1 = {nullptr, 0}, Blk y1 = {nullptr, 0}, Blk x2 = {nullptr, 0}, Blk y2 = {nullptr, 0})
{
    MDotArgs a{p->n, p->cells, p->s, {x0.p, x1.p, x2.p}, {y0.p, y1.p, y2.p}, {x0.ld, x1.ld, x2.ld}, {y0.ld, y1.ld, y2.ld}, p->part};
    launch_dot(st, x2.p ? 3 : x1.p ? 2 : 1, a);
}

void fold(const MultiPlan *p, hipStream_t st, int op, int nd, int flag, double rtol = 0.0, double atol = 0.0, int64_t max_iter = 0)
{
    launch_fold(st, op, nd, flag, p->s, p->cells, p->part, p->blk, nullptr, rtol, atol, max_iter);
}

int pcg_iteration(const MultiPlan *p, hipStream_t st)
{
    const bool jac = p->pre.jacobi(), app = p->pre.applied();
    const int64_t s = p->s;
    const Blk x{p->x, p->ldx}, r{p->w(V_R), s}, pp{p->w(V_P), s}, q{p->w(V_Q), s}, z{p->pre.none() ? p->w(V_R) : p->w(V_Z), s};
    const Blk dinv{const_cast<double *>(p->dinv()), 0};
    int rc = product(p, st, pp.p, s, q.p);
    if (rc != SBLAS_OK) return rc;
    dot(p, st, pp, q);
    fold(p, st, FOLD_PCG_ALPHA, 1, 0);
    launch_update(st, SBLAS_KRYLOV_UP_PCG_XR, jac, up_args(p, {x, r, pp, q, dinv, z}));
    fold(p, st, FOLD_PCG_RES, jac ? 2 : 1, !app);
    if (app) { // krylov.hip's applied sequence, column-wise: on all columns, into Z only
        if ((rc = p->pre.apply_multi(st, p->s, r.p, s, z.p, s)) != SBLAS_OK) return rc;
        dot(p, st, r, z);
        fold(p, st, FOLD_PCG_BETA, 1, 0);
    }
    launch_update(st, SBLAS_KRYLOV_UP_PCG_P, false, up_args(p, {pp, z}));
    return SBLAS_OK;
}

int bicgstab_iteration(const MultiPlan *p, hipStream_t st)
{
    const bool jac = p->pre.jacobi(), none = p->pre.none(), app = p->pre.applied();
    const int64_t s = p->s;
    const Blk x{p->x, p->ldx}, r{p->w(B_R), s}, rh{p->w(B_RHAT), s}, pp{p->w(B_P), s}, v{p->w(B_V), s}, sv{p->w(B_S), s}, t{p->w(B_T), s};
    const Blk ph = none ? pp : Blk{p->w(B_PH), s}, sh = none ? sv : Blk{p->w(B_SH), s}, dinv{const_cast<double *>(p->dinv()), 0};
    int rc;
    launch_update(st, SBLAS_KRYLOV_UP_BICG_P, jac, up_args(p, {pp, r, v, dinv, ph}));
    if (app && (rc = p->pre.apply_multi(st, p->s, pp.p, s, ph.p, s)) != SBLAS_OK) return rc;
    if ((rc = product(p, st, ph.p, s, v.p)) != SBLAS_OK) return rc;
    dot(p, st, rh, v);
    fold(p, st, FOLD_BICG_ALPHA, 1, 0);
    launch_update(st, SBLAS_KRYLOV_UP_BICG_S, jac, up_args(p, {sv, r, v, dinv, sh}));
    if (app && (rc = p->pre.apply_multi(st, p->s, sv.p, s, sh.p, s)) != SBLAS_OK) return rc;
    if ((rc = product(p, st, sh.p, s, t.p)) != SBLAS_OK) return rc;
    dot(p, st, t, sv, t, t, sv, sv);
    fold(p, st, FOLD_BICG_OMEGA, 3, 0);
    launch_update(st, SBLAS_KRYLOV_UP_BICG_XR, false, up_args(p, {x, r, ph, sh, sv, t, rh}));
    fold(p, st, FOLD_BICG_RES, 2, 0);
    return SBLAS_OK;
}

// launches of one iteration without the products': through the rule of the seat's kind
int64_t iteration_launches(const MultiPlan *p)
{
    const int kind = p->pre.kind;
    if (precond_multi_pair(kind)) {
        int64_t lower[12], upper[12];
        p->pre.info(lower, upper);
        return sblas_krylov_multi_launches_pair(p->method, kind, 0, lower[5], upper[5]);
    }
    int64_t mi[4] = {0, 0, 0, 0};
    if (precond_multi_applied(kind)) sblas_hip_amg_plan_multi_info(p->pre.lower, mi);
    return sblas_krylov_multi_launches_ex(p->method, kind, 0, mi[2]);
}

// the three creates.  precond_plan: the plan of an applied kind (create_ex), or with upper_plan the lower one of a pair
// of solve plans (create_pair); multi_bind seats either.  The work blocks an applied kind writes -- Z, P^ and S^ -- are
// among the plan's own already.
int create_plan(int dev, void *stream, int method, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx, int nrhs, int precond,
                const void *precond_plan, const void *upper_plan, void **plan_out)
{
    if (!krylov_multi_width_ok(nrhs)) return SBLAS_E_INVALID;
    std::unique_ptr<MultiPlan> p(new MultiPlan);
    p->method = method;
    int rc = multi_bind(p.get(), dev, stream, n, nnz, rowptr, colidx, nrhs, precond, precond_plan, upper_plan);
    if (rc != SBLAS_OK) return rc;
    p->n_blocks = method == SBLAS_KRYLOV_PCG ? KRYLOV_PCG_VECTORS : KRYLOV_BICGSTAB_VECTORS;
    rc = multi_layout(p.get(), stream, {{&p->blk, &p->scalar_bytes, (size_t)nrhs * KRYLOV_BLOCK_SLOTS * 8, 1},
                                        {&p->part, &p->partial_bytes, (size_t)KRYLOV_MAX_DOTS * (size_t)nrhs * (size_t)p->cells * 8, 1},
                                        multi_workspace(p.get()),
                                        {&p->vec, &p->block_bytes, (size_t)n * (size_t)nrhs * 8, p->n_blocks}});
    if (rc != SBLAS_OK) return rc;
    *plan_out = p.release();
    return SBLAS_OK;
}

} // namespace

extern "C" {

size_t sblas_hip_krylov_multi_dot_workspace(int64_t n, int nrhs, int ndots)
{
    if (n < 0 || !krylov_multi_width_ok(nrhs) || ndots < 1 || ndots > KRYLOV_MAX_DOTS) return 0;
    const size_t sums = (size_t)ndots * (size_t)nrhs * (size_t)krylov_cells(n);
    return (sums ? sums : 1) * sizeof(double); // never 0: a workspace is always asked for
}

int sblas_hip_krylov_multi_dot_f64(int dev, void *stream, int64_t n, int nrhs, int ndots, const double *const *x, const int64_t *ldx,
                                   const double *const *y, const int64_t *ldy, double *out, void *workspace, size_t workspace_bytes)
{
    if (n < 0 || n > INT_MAX || !krylov_multi_width_ok(nrhs) || ndots < 1 || ndots > KRYLOV_MAX_DOTS) return SBLAS_E_INVALID;
    if (!x || !y || !ldx || !ldy || !out) return SBLAS_E_INVALID;
    for (int q = 0; q < ndots; ++q) {
        if (n > 0 && (!x[q] || !y[q])) return SBLAS_E_INVALID;
        if (ldx[q] < nrhs || ldy[q] < nrhs) return SBLAS_E_INVALID;
        if (n > 0 && ((reinterpret_cast<uintptr_t>(x[q]) | reinterpret_cast<uintptr_t>(y[q])) & 7u)) return SBLAS_E_INVALID;
    }
    if (!workspace || workspace_bytes < sblas_hip_krylov_multi_dot_workspace(n, nrhs, ndots)) return SBLAS_E_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(out)) & 7u) return SBLAS_E_INVALID;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    hipStream_t st = (hipStream_t)stream;
    MDotArgs a{n, krylov_cells(n), nrhs, {}, {}, {}, {}, static_cast<double *>(workspace)};
    for (int q = 0; q < ndots; ++q) a.x[q] = x[q], a.y[q] = y[q], a.ldx[q] = ldx[q], a.ldy[q] = ldy[q];
    if (a.cells > 0) launch_dot(st, ndots, a);
    launch_fold(st, FOLD_OUT, ndots, 0, nrhs, a.cells, a.part, nullptr, out);
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_krylov_multi_update_f64(int dev, void *stream, int op, int jacobi, int64_t n, int nrhs, const double *scalars,
                                      double *const *v, const int64_t *ld, int nv, double *partial)
{
    static const int parts[5] = {1, 0, 0, 0, 2};
    if (op < SBLAS_KRYLOV_UP_PCG_XR || op > SBLAS_KRYLOV_UP_BICG_XR || n < 0 || n > INT_MAX || !krylov_multi_width_ok(nrhs)) return SBLAS_E_INVALID;
    if (!scalars || !v || !ld || (reinterpret_cast<uintptr_t>(scalars) & 7u)) return SBLAS_E_INVALID;
    const bool jac = dinv_place(op, jacobi != 0) >= 0;
    const int want = blocks_of(op, jac), dp = dinv_place(op, jac);
    if (nv < want || nv > 8) return SBLAS_E_INVALID;
    for (int q = 0; q < want; ++q) {
        if (q != dp && ld[q] < nrhs) return SBLAS_E_INVALID;
        if (n > 0 && (!v[q] || (reinterpret_cast<uintptr_t>(v[q]) & 7u))) return SBLAS_E_INVALID;
    }
    if (n == 0) return SBLAS_OK;
    if (parts[op] && (!partial || (reinterpret_cast<uintptr_t>(partial) & 7u))) return SBLAS_E_INVALID;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    MUpArgs a{n, krylov_cells(n), nrhs, const_cast<double *>(scalars), partial, {}, {}};
    for (int q = 0; q < want; ++q) a.v[q] = v[q], a.ld[q] = q == dp ? 0 : ld[q];
    launch_update((hipStream_t)stream, op, jac, a);
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_krylov_multi_plan_create(int dev, void *stream, int method, int64_t n, int64_t nnz, const int32_t *rowptr,
                                       const int32_t *colidx, int nrhs, int precond, void **plan_out)
{
    if (!plan_out) return SBLAS_E_INVALID;
    *plan_out = nullptr;
    if (method != SBLAS_KRYLOV_PCG && method != SBLAS_KRYLOV_BICGSTAB) return SBLAS_E_INVALID;
    if (!precond_multi(precond)) return SBLAS_E_INVALID; // precond_rule.h: an applied kind needs its plan, which create_ex takes
    return create_plan(dev, stream, method, n, nnz, rowptr, colidx, nrhs, precond, nullptr, nullptr, plan_out);
}

int sblas_hip_krylov_multi_plan_create_ex(int dev, void *stream, int method, int64_t n, int64_t nnz, const int32_t *rowptr,
                                          const int32_t *colidx, int nrhs, int precond, void *precond_plan, void **plan_out)
{
    if (!plan_out) return SBLAS_E_INVALID;
    *plan_out = nullptr;
    if (method != SBLAS_KRYLOV_PCG && method != SBLAS_KRYLOV_BICGSTAB) return SBLAS_E_INVALID;
    // precond_rule.h: a kind that rides in the kernels takes no plan, AMG takes its own, every other kind is refused
    if (precond_multi(precond) ? precond_plan != nullptr : !(precond_multi_applied(precond) && precond_plan)) return SBLAS_E_INVALID;
    return create_plan(dev, stream, method, n, nnz, rowptr, colidx, nrhs, precond, precond_plan, nullptr, plan_out);
}

int sblas_hip_krylov_multi_plan_create_pair(int dev, void *stream, int method, int64_t n, int64_t nnz, const int32_t *rowptr,
                                            const int32_t *colidx, int nrhs, const void *lower_plan, const void *upper_plan, void **plan_out)
{
    if (!plan_out) return SBLAS_E_INVALID;
    *plan_out = nullptr;
    if (method != SBLAS_KRYLOV_PCG && method != SBLAS_KRYLOV_BICGSTAB) return SBLAS_E_INVALID;
    if (!lower_plan || !upper_plan) return SBLAS_E_INVALID;
    return create_plan(dev, stream, method, n, nnz, rowptr, colidx, nrhs, SBLAS_PRECOND_ILU0, lower_plan, upper_plan, plan_out);
}

int sblas_hip_krylov_multi_plan_info(const void *plan, int64_t out[12])
{
    if (!plan || !out) return SBLAS_E_INVALID;
    const MultiPlan *p = static_cast<const MultiPlan *>(plan);
    out[0] = p->n, out[1] = p->nnz, out[2] = p->method, out[3] = p->pre.kind, out[4] = p->s, out[5] = p->n_blocks;
    out[6] = (int64_t)p->block_bytes, out[7] = (int64_t)p->partial_bytes, out[8] = (int64_t)p->scalar_bytes, out[9] = (int64_t)p->ws_bytes;
    out[10] = (int64_t)p->bytes, out[11] = iteration_launches(p);
    return SBLAS_OK;
}

int sblas_hip_krylov_multi_plan_destroy(void *plan)
{
    delete static_cast<MultiPlan *>(plan);
    return SBLAS_OK;
}

int sblas_hip_krylov_multi_start(void *plan, void *stream, const double *val, const double *dinv, const double *B, int64_t ldb, double *X,
                                 int64_t ldx, double rtol, double atol, int64_t max_iter)
{
    MultiPlan *p = static_cast<MultiPlan *>(plan);
    const MultiStart go = multi_start(p, val, dinv, B, ldb, X, ldx, rtol, atol, max_iter); // dinv carries the factor lu of a pair
    if (go != MULTI_GO) return go == MULTI_EMPTY ? SBLAS_OK : SBLAS_E_INVALID;
    const bool jac = p->pre.jacobi();
    hipStream_t st = (hipStream_t)stream;
    const bool pcg = p->method == SBLAS_KRYLOV_PCG;
    const int64_t s = p->s;
    const Blk b{const_cast<double *>(B), ldb}, x{X, ldx}, di{const_cast<double *>(p->dinv()), 0};
    int rc;
    // The work blocks start every solve from zero.  A column that is frozen from the start is never written, yet the SpMM
    // multiplies it -- and a non-finite value a previous solve left there would select other SpMM kernels for the whole
    // product.  So the bits of a solve are a function of its own operands alone.
    if (hipMemsetAsync(p->vec, 0, (size_t)p->n_blocks * p->block_bytes, st) != hipSuccess) return SBLAS_E_HIP;
    dot(p, st, b, b);
    fold(p, st, FOLD_START_B, 1, !pcg, rtol, atol, max_iter);
    if (pcg) {
        const Blk r{p->w(V_R), s}, q{p->w(V_Q), s}, z{p->pre.none() ? p->w(V_R) : p->w(V_Z), s}, pp{p->w(V_P), s};
        if ((rc = product(p, st, X, ldx, q.p)) != SBLAS_OK) return rc;
        launch_update(st, UP_START_PCG, jac, up_args(p, {r, b, q, di, z, x}));
        fold(p, st, FOLD_START_R, jac ? 2 : 1, 0);
        if (p->pre.applied()) { // krylov.hip's start: z = M^-1 r on all columns, then rho = (r, z)
            if ((rc = p->pre.apply_multi(st, p->s, r.p, s, z.p, s)) != SBLAS_OK) return rc;
            dot(p, st, r, z);
            fold(p, st, FOLD_RHO0, 1, 0);
        }
        launch_update(st, UP_COPY, false, up_args(p, {pp, z}));
    } else {
        const Blk r{p->w(B_R), s}, v{p->w(B_V), s}, rh{p->w(B_RHAT), s}, pp{p->w(B_P), s};
        if ((rc = product(p, st, X, ldx, v.p)) != SBLAS_OK) return rc;
        launch_update(st, UP_START_BICG, false, up_args(p, {r, b, v, rh, pp, x}));
        fold(p, st, FOLD_START_R, 1, 0);
    }
    if (hipGetLastError() != hipSuccess) return SBLAS_E_HIP;
    p->started = true;
    return SBLAS_OK;
}

int sblas_hip_krylov_multi_iterate(void *plan, void *stream, int64_t k)
{
    const MultiPlan *p = static_cast<const MultiPlan *>(plan);
    if (!p || k < 0 || !p->started) return SBLAS_E_INVALID;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    if (p->n == 0) return SBLAS_OK;
    hipStream_t st = (hipStream_t)stream;
    for (int64_t it = 0; it < k; ++it) {
        const int rc = p->method == SBLAS_KRYLOV_PCG ? pcg_iteration(p, st) : bicgstab_iteration(p, st);
        if (rc != SBLAS_OK) return rc;
    }
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_krylov_multi_status(const void *plan, void *stream, double *out)
{
    static const StatusSlot table[8] = {{KS_STATUS, true}, {KS_ITER, true}, {KS_RNORM, false}, {KS_BNORM, false},
                                        {KS_ALPHA, false}, {KS_BETA, false}, {KS_OMEGA, false}, {KS_WHICH, true}};
    return multi_status<KRYLOV_BLOCK_SLOTS>(static_cast<const MultiPlan *>(plan), stream, out, table);
}

} // extern "C"
